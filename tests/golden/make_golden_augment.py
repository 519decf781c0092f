#!/usr/bin/env python3
"""Generates tests/golden/augment_ref.npz from the REAL reference's YCB-V loader (datasets/ycbv/ycbv_pbr.py).

Runs ONLY where the reference tree is mounted; nothing here travels anywhere except the .npz it writes.  The text of the two methods
is read from the mounted tree at generation time, executed, and never stored:
  gaussian_noise (:292-296)   img + rng.randn(*img.shape) * sigma, clipped to 0 .. 255 and cast to uint8.  The stub generator hands
                              it integer noise divided by sigma = 8, so that the sum is an integer and the fixture pins the clip.
  add_real_back (:355-387)    the whole method; its three PIL reads are answered by arrays (a stub `Image.open`), its three randint
                              calls by the stored window and frame index.

Contents:
  gn_img u8[24,24,3], gn_noise i64[24,24,3], gn_sigma, gn_out u8[24,24,3]
  rb_rgb u8[S,S,3], rb_labels u8[S,S], rb_dpt f32[S,S], rb_dpt_msk u8[S,S]      the crop (S = 32)
  rb_bg_rgb u8[2,48,56,3], rb_bg_depth_raw u16[2,48,56], rb_bg_depth f32[2,48,56] (raw / 1000 in fp64, cast), rb_bg_mask u8[2,48,56]
  rb_draws = (rnd_h, rnd_w, frame);  rb_out_rgb u8[S,S,3], rb_out_dpt f32[S,S]
"""
import ast
import os
import textwrap

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


def grab_methods(rel_path, names):
    """The dedented source text of the named methods, whichever class of the file holds them."""
    text = open(os.path.join(REF, rel_path)).read()
    lines = text.split("\n")
    out = {}
    for node in ast.walk(ast.parse(text)):
        if isinstance(node, ast.FunctionDef) and node.name in names and node.name not in out:
            out[node.name] = textwrap.dedent("\n".join(lines[node.lineno - 1:node.end_lineno]))
    assert sorted(out) == sorted(names), (rel_path, names)
    return out


class _Arr:
    def __init__(self, a):
        self.a = a

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def __array__(self, dtype=None, copy=None):
        return self.a if dtype is None else self.a.astype(dtype)


class _Image:
    def __init__(self, files):
        self.files = files

    def open(self, name):
        return _Arr(self.files[name])


class _Rng:
    def __init__(self, ints=(), normal=None):
        self.ints, self.normal = list(ints), normal

    def randint(self, *a):
        return self.ints.pop(0)

    def randn(self, *shape):
        assert tuple(shape) == self.normal.shape
        return self.normal


class _Self:
    pass


def main():
    assert os.path.isdir(REF), "reference tree not mounted"
    src = grab_methods("datasets/ycbv/ycbv_pbr.py", ["gaussian_noise", "add_real_back"])
    rs = np.random.RandomState(5)
    out = {}

    ns = dict(np=np)
    exec(src["gaussian_noise"], ns)
    img = rs.randint(0, 256, size=(24, 24, 3)).astype(np.uint8)
    noise = rs.randint(-300, 301, size=img.shape).astype(np.int64)
    sigma = 8
    out.update(gn_img=img, gn_noise=noise, gn_sigma=np.int64(sigma),
               gn_out=ns["gaussian_noise"](None, _Rng(normal=noise / float(sigma)), img, sigma))

    S, Nb, Hb, Wb = 32, 2, 48, 56
    bg_rgb = rs.randint(0, 256, size=(Nb, Hb, Wb, 3)).astype(np.uint8)
    bg_raw = (rs.randint(300, 3000, size=(Nb, Hb, Wb)) * (rs.rand(Nb, Hb, Wb) > 0.2)).astype(np.uint16)
    bg_mask = rs.choice(np.array([0, 3, 254, 255], np.uint8), size=(Nb, Hb, Wb))
    rgb = rs.randint(0, 256, size=(S, S, 3)).astype(np.uint8)
    labels = rs.choice(np.array([0, 0, 1, 255], np.uint8), size=(S, S))
    dpt = (rs.uniform(0.3, 2.0, size=(S, S)) * (rs.rand(S, S) > 0.4)).astype(np.float32)
    dpt_msk = (dpt > 1e-6).astype(np.uint8)
    draws = (Hb - S - 2, 7, 1)                                   # rnd_h (the largest the exclusive randint gives), rnd_w, frame
    me = _Self()
    me.im_h, me.im_w, me.in_size = Hb, Wb, S
    me.rng = _Rng(ints=draws)
    me.real_annos = [dict(depth_factor=1000.0, depth_file="d%d" % i, mask_file="m%d" % i, rgb_file="c%d" % i) for i in range(Nb)]
    files = {}
    for i in range(Nb):
        files.update({"d%d" % i: bg_raw[i], "m%d" % i: bg_mask[i], "c%d" % i: bg_rgb[i]})
    ns = dict(np=np, Image=_Image(files))
    exec(src["add_real_back"], ns)
    o_rgb, o_dpt = ns["add_real_back"](me, rgb, labels, dpt, dpt_msk)
    assert o_rgb.dtype == np.uint8 and o_dpt.dtype == np.float32
    out.update(rb_rgb=rgb, rb_labels=labels, rb_dpt=dpt, rb_dpt_msk=dpt_msk, rb_bg_rgb=bg_rgb, rb_bg_depth_raw=bg_raw,
               rb_bg_depth=(bg_raw / 1000.0).astype(np.float32), rb_bg_mask=bg_mask, rb_draws=np.asarray(draws, np.int64),
               rb_out_rgb=o_rgb, rb_out_dpt=o_dpt)
    np.savez_compressed(os.path.join(HERE, "augment_ref.npz"), **out)
    print("augment_ref.npz: %d of %d pixels pasted, %d depths pasted" %
          ((labels == 0).sum(), S * S, (dpt_msk == 0).sum()))


if __name__ == "__main__":
    main()
