"""CPU: the written rule of the crop augmentation (include/gdm.h gdm_augment_crops_hip) as frontend.augment_crops_numpy
restates it, its committed tables, the hash-drawn box jitter, and the two places where the rule can be held against the reference's own
statements (tests/golden/augment_ref.npz, written by make_golden_augment.py where the reference tree is mounted)."""
import importlib.util
import os

import numpy as np
import torch

from geometric_aware_dense_matching_amd import frontend as fe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def _tool():
    spec = importlib.util.spec_from_file_location("make_aug_tables", os.path.join(ROOT, "tools", "make_aug_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_level_recovery_is_exact_for_all_3x256_values():
    f32 = np.float32
    lv = np.broadcast_to(np.arange(256).reshape(1, 256, 1), (3, 256, 1))
    x = fe.aug_normalise(lv)
    assert x.dtype == np.float32 and np.array_equal(fe.aug_levels(x), lv)
    mean, std = np.array(fe.COLOR_MEAN, f32).reshape(3, 1, 1), np.array(fe.COLOR_STD_CROP, f32).reshape(3, 1, 1)
    back = (((x * std) + mean) * f32(255.0)).astype(np.float64)
    dist = np.abs(back - lv).max()
    print("largest distance of a recovered level from its integer: %.3g" % dist)
    assert dist < 1e-4                                             # 1.5e-5 measured; rintf needs < 0.5
    assert np.array_equal(fe.aug_levels(np.full((3, 1, 1), np.nan, f32)), np.zeros((3, 1, 1)))
    assert np.array_equal(fe.aug_levels(np.full((3, 1, 1), 1e9, f32)), np.full((3, 1, 1), 255))


def test_tables_equal_their_formula():
    tool, t = _tool(), fe.aug_tables()
    assert open(os.path.join(ROOT, "geometric_aware_dense_matching_amd", "csrc", "gdm_augment_tables.h")).read() == tool.render()
    want = tool.tables()
    assert sorted(t) == sorted(want) and all(np.array_equal(t[k], np.asarray(want[k])) for k in want)
    g3, g5 = t["gdm_aug_gauss3"], t["gdm_aug_gauss5"]
    assert ((g3[:, 0] + 2 * g3[:, 1]) == 256).all() and ((g5[:, 0] + 2 * g5[:, 1] + 2 * g5[:, 2]) == 256).all()
    assert (g3 >= 0).all() and (g5 >= 0).all()
    # level 0 is OpenCV's sigma for the kernel size, 0.8 and 1.1
    for k, row in ((3, g3[0]), (5, g5[0])):
        sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
        g = np.exp(-np.arange(k // 2 + 1) ** 2 / (2 * sigma * sigma))
        assert np.array_equal(row[1:], np.rint(256 * g[1:] / (g[0] + 2 * g[1:].sum())))
    cos = t["gdm_aug_cos_q14"]
    assert cos[0] == 16384 and cos[90] == 0 and cos[180] == -16384 and cos[45] == 11585 and np.array_equal(cos[1:], cos[1:][::-1])


def test_draw_constants_differ_from_the_other_streams():
    assert fe.AUG_C != 0x9e3779b9 and fe.DZI_C != 0x9e3779b9 and fe.AUG_C != fe.DZI_C


def test_draws_follow_the_written_ranges_and_rates():
    d = fe.augment_draws_numpy(4000, 11, S=64, bank_shape=(5, 80, 96))
    p0 = [x["passes"][0] for x in d]
    assert min(p["ks"] for p in p0) == 320 and max(p["ks"] for p in p0) == 371
    assert min(p["kv"] for p in p0) == 294 and max(p["kv"] for p in p0) == 345
    assert min(p["length"] for p in p0) == 1 and max(p["length"] for p in p0) == 15
    assert min(p["angle"] for p in p0) == 0 and max(p["angle"] for p in p0) == 359
    assert all(1 <= p["a"] <= 30 and 1 <= len(p["taps"]) <= 16 and p["halo"] <= 18 for p in p0)
    assert max(p["sigma"] for p in p0) == 24 and min(p["sigma"] for p in p0) == 0
    for key in ("sharpen", "motion", "gauss", "extra"):
        rate = np.mean([p[key] for p in p0])
        assert abs(rate - 0.2) < 0.03, (key, rate)                 # 4 standard deviations of a 4000-draw rate are 0.025
    assert abs(np.mean([x["second"] for x in d]) - 0.2) < 0.03
    assert abs(np.mean([p["gauss_k"] == 3 for p in p0]) - 0.8) < 0.03
    assert all(0 <= x["bank"] < 5 and 0 <= x["wy"] < 80 - 64 - 1 and 0 <= x["wx"] < 96 - 64 - 1 for x in d)
    assert max(x["wy"] for x in d) == 14 and max(x["wx"] for x in d) == 30


def test_hsv_gain_identity_and_grey():
    M, m, c = np.meshgrid(np.arange(256), np.arange(256), np.arange(0, 256, 5), indexing="ij")
    ok = (m <= c) & (c <= M)
    img = np.stack([M[ok], c[ok], m[ok]], axis=1)[None]           # every (max, min) pair, the middle channel in steps of 5
    assert np.array_equal(fe.aug_hsv_gain(img, 256, 256), img)     # gains 256/256: the identity
    out = fe.aug_hsv_gain(img, 371, 345)
    assert out.min() >= 0 and out.max() <= 255
    assert (out[..., 0] >= out[..., 1]).all() and (out[..., 1] >= out[..., 2]).all()       # the channel order is kept
    grey = np.repeat(np.arange(256).reshape(1, 256, 1), 3, axis=2)
    g = fe.aug_hsv_gain(grey, 350, 300)
    assert (g[..., 0] == g[..., 1]).all() and (g[..., 1] == g[..., 2]).all()
    assert np.array_equal(g[0, :, 0], np.minimum(255, (np.arange(256) * 300) >> 8))


def test_all_stages_off_is_the_identity():
    rs = np.random.RandomState(0)
    img = rs.randint(0, 256, size=(40, 40, 3)).astype(np.int64)
    p = dict(ks=256, kv=256, sharpen=False, motion=False, gauss=False, sigma=0, extra=False, hs=(1, 2))
    assert np.array_equal(fe.aug_pass(img, p), img)


def test_constant_image_survives_every_stencil():
    t = fe.aug_tables()
    for v in (0, 1, 77, 254, 255):
        img = np.full((33, 35, 3), v, np.int64)
        for u in (0, 100, 255):
            assert np.array_equal(fe.aug_sharpen(img, u), img)
        for angle, length in ((0, 15), (37, 9), (90, 1), (200, 15), (315, 4)):
            assert np.array_equal(fe.aug_motion(img, fe.motion_taps(angle, length)[1]), img)
        for lvl in (0, 1, 60, 128, 255):
            assert np.array_equal(fe.aug_gauss(img, list(t["gdm_aug_gauss3"][lvl])), img)
            assert np.array_equal(fe.aug_gauss(img, list(t["gdm_aug_gauss5"][lvl])), img)


def test_stencils_on_a_small_image_by_hand():
    img = np.zeros((32, 32, 3), np.int64)
    img[0, 0] = 200                                                # a corner: REFLECT_101 mirrors about the border pixel
    s = fe.aug_sharpen(img, 0)                                     # c = 9, divided by 1
    assert s[0, 0, 0] == 255 and s[1, 1, 0] == 0 and s[0, 1, 0] == 0
    img[:] = 0
    img[5, 5] = 60
    s = fe.aug_sharpen(img, 255)                                   # c256 = 3069, q = 1021
    assert s[5, 5, 0] == (2 * 3069 * 60 + 1021) // (2 * 1021) == 180 and s[5, 6, 0] == 0
    img[5, 5] = 90
    g = fe.aug_gauss(img, [128, 64])
    assert g[5, 5, 0] == (128 * 128 * 90 + 32768) >> 16 and g[4, 4, 0] == (64 * 64 * 90 + 32768) >> 16 and g[5, 7, 0] == 0
    m = fe.aug_motion(img, [(0, 0), (0, 1), (0, 2)])
    assert m[5, 5, 0] == 30 and m[5, 3, 0] == 30 and m[5, 6, 0] == 0 and m[5, 2, 0] == 0


def test_motion_kernel_row_column_diagonal():
    assert fe.motion_taps(0, 4) == (8, [(0, 0), (0, 1), (0, 2), (0, 3)])                   # the end point x = 8 falls outside the kernel
    assert fe.motion_taps(90, 4) == (8, [(0, 0), (1, 0), (2, 0), (3, 0)])
    assert fe.motion_taps(45, 6) == (8, [(0, 0), (1, 1), (2, 2), (3, 3)])
    assert fe.motion_taps(180, 3) == (6, [(0, 0), (0, -1), (0, -2), (0, -3)])
    assert fe.motion_taps(45, 1) == (1, [(0, 0)])                                          # a 1 x 1 kernel
    assert fe.motion_taps(0, 0) == (0, None)                                               # a <= 0: the early return (length 0 is never drawn)
    for angle in range(360):
        for length in (1, 7, 15):
            a, taps = fe.motion_taps(angle, length)
            assert 1 <= a <= 30 and 1 <= len(taps) <= 16 and len(set(taps)) == len(taps)
            assert all(-(a // 2) <= d <= a - 1 - a // 2 and abs(d) <= 15 for tap in taps for d in tap)


def test_noise_standard_deviation():
    img = np.full((256, 256, 3), 128, np.int64)
    for sigma in (7, 24):
        # |z| <= 510, so the noise is at most (510 * 24 * 443 + 32768) >> 16 = 83 < 127: clipping cannot bite
        assert (510 * sigma * 443 + 32768) >> 16 < 127
        out = fe.aug_noise(img, sigma, 0x1234567)
        assert out.min() > 0 and out.max() < 255
        sd = (out - 128).std()
        print("sigma %d: measured %.4f" % (sigma, sd))
        assert abs(sd - sigma) < 0.02 * sigma and abs((out - 128).mean()) < 0.1
    assert np.array_equal(fe.aug_noise(img, 0, 5), img)
    assert fe.aug_noise(np.full((32, 32, 3), 250, np.int64), 24, 9).max() == 255


def _crops(B, S, seed):
    rs = np.random.RandomState(seed)
    rgb = fe.aug_normalise(rs.randint(0, 256, size=(B, 3, S, S)))
    depth = (rs.uniform(0.3, 2.0, size=(B, S, S)) * (rs.rand(B, S, S) > 0.4)).astype(np.float32)
    mask = rs.choice(np.array([0, 0, 3, 255], np.uint8), size=(B, S, S))
    bank = (rs.randint(0, 256, size=(2, S + 9, S + 20, 3)).astype(np.uint8), rs.uniform(0.5, 3.0, size=(2, S + 9, S + 20)).astype(np.float32),
            rs.choice(np.array([0, 9, 255], np.uint8), size=(2, S + 9, S + 20)))
    return rgb, depth, mask, bank


def test_enable_zero_returns_the_input_bits():
    rgb, depth, mask, bank = _crops(3, 32, 1)
    rgb[1, 0, 0, 0] = np.float32(0.123456)                         # no level: only a bit copy returns it
    o_rgb, o_depth = fe.augment_crops_numpy(rgb, depth, mask, bank, np.array([1, 0, 1], np.uint8), seed=4)
    assert np.array_equal(o_rgb[1].view(np.uint32), rgb[1].view(np.uint32)) and np.array_equal(o_depth[1], depth[1])
    assert not np.array_equal(o_rgb[0], rgb[0]) and not np.array_equal(o_depth[0], depth[0])
    full = fe.augment_crops_numpy(rgb, depth, mask, bank, None, seed=4)
    assert np.array_equal(full[0][0], o_rgb[0]) and np.array_equal(full[0][2], o_rgb[2]) and not np.array_equal(full[0][1], rgb[1])


def test_paste_keeps_object_and_valid_depth_and_takes_the_window():
    B, S = 4, 32
    rgb, depth, mask, bank = _crops(B, S, 2)
    seed = next(s for s in range(100) if not any(d["second"] for d in fe.augment_draws_numpy(B, s)))
    draws = fe.augment_draws_numpy(B, seed, S, bank[0].shape[:3])
    o_rgb, o_depth = fe.augment_crops_numpy(rgb, depth, mask, bank, None, seed=seed)
    plain, plain_depth = fe.augment_crops_numpy(rgb, depth, mask, None, None, seed=seed)
    assert np.array_equal(plain_depth, depth)
    for b, d in enumerate(draws):
        win = (slice(d["wy"], d["wy"] + S), slice(d["wx"], d["wx"] + S))
        keep = bank[2][d["bank"]][win] < 255
        obj = mask[b] > 0
        lv = fe.aug_levels(o_rgb[b]).transpose(1, 2, 0)
        assert np.array_equal(lv[obj], fe.aug_levels(plain[b]).transpose(1, 2, 0)[obj])                # the object: pass 0 alone
        assert np.array_equal(lv[~obj & keep], bank[0][d["bank"]][win][~obj & keep])
        assert not lv[~obj & ~keep].any()
        valid = depth[b] > 1e-6
        assert np.array_equal(o_depth[b][valid], depth[b][valid])
        assert np.array_equal(o_depth[b][~valid & keep], bank[1][d["bank"]][win][~valid & keep]) and not o_depth[b][~valid & ~keep].any()
        assert obj.any() and (~obj & keep).any() and (~obj & ~keep).any() and (~valid & keep).any()


def test_whole_call_is_levels_pass_paste_pass_normalise():
    B, S = 6, 40
    rgb, depth, mask, bank = _crops(B, S, 3)
    seed = next(s for s in range(200) if sum(d["second"] for d in fe.augment_draws_numpy(B, s)) >= 2)
    o_rgb, o_depth = fe.augment_crops_numpy(rgb, depth, mask, bank, None, seed=seed)
    for b, d in enumerate(fe.augment_draws_numpy(B, seed, S, bank[0].shape[:3])):
        img = fe.aug_pass(fe.aug_levels(rgb[b]).transpose(1, 2, 0), d["passes"][0])
        img, dep = fe.aug_paste(img, depth[b], mask[b], *bank, d["bank"], d["wy"], d["wx"])
        if d["second"]:
            img = fe.aug_pass(img, d["passes"][1])
        assert np.array_equal(o_rgb[b], fe.aug_normalise(img.transpose(2, 0, 1))) and np.array_equal(o_depth[b], dep)
    again = fe.augment_crops_numpy(rgb, depth, mask, bank, None, seed=seed)
    assert np.array_equal(again[0], o_rgb) and np.array_equal(again[1], o_depth)
    other = fe.augment_crops_numpy(rgb, depth, mask, bank, None, seed=seed + 1)
    assert not np.array_equal(other[0], o_rgb)


def test_against_the_reference_statements():
    g = np.load(os.path.join(G, "augment_ref.npz"))
    # gaussian_noise: integer noise, so the fixture pins the clip of step 5
    assert np.array_equal(np.clip(g["gn_img"].astype(np.int64) + g["gn_noise"], 0, 255), g["gn_out"])
    assert (g["gn_img"].astype(np.int64) + g["gn_noise"]).min() < 0 and (g["gn_img"].astype(np.int64) + g["gn_noise"]).max() > 255
    # add_real_back: the compositing of colour and depth
    rnd_h, rnd_w, frame = (int(v) for v in g["rb_draws"])
    assert np.array_equal(g["rb_dpt_msk"] > 0, g["rb_dpt"] > 1e-6)                           # the crop's depth mask is depth > 1e-6
    img, dep = fe.aug_paste(g["rb_rgb"].astype(np.int64), g["rb_dpt"], g["rb_labels"], g["rb_bg_rgb"], g["rb_bg_depth"], g["rb_bg_mask"],
                            frame, rnd_h, rnd_w)
    assert np.array_equal(img, g["rb_out_rgb"]) and np.array_equal(dep, g["rb_out_dpt"])
    assert not np.array_equal(g["rb_out_rgb"], g["rb_rgb"]) and not np.array_equal(g["rb_out_dpt"], g["rb_dpt"])


def test_small_crops_and_small_banks_are_refused():
    import pytest
    rgb, depth, mask, bank = _crops(1, 32, 4)
    with pytest.raises(ValueError):
        fe.augment_crops_numpy(rgb[:, :, :31, :31], depth[:, :31, :31], mask[:, :31, :31])
    with pytest.raises(ValueError):
        fe.augment_crops_numpy(rgb, depth, mask, tuple(a[:, :33] for a in bank))
    with pytest.raises(ValueError):
        fe.augment_crops_numpy(rgb, depth, None, bank)


def test_dzi_boxes_numpy_equals_the_torch_arithmetic_on_the_same_numbers():
    rs = np.random.RandomState(7)
    B = 257
    x1, y1 = rs.uniform(0, 400, B), rs.uniform(0, 300, B)
    box = np.stack([x1, y1, x1 + rs.uniform(5, 600, B), y1 + rs.uniform(5, 600, B)], axis=1).astype(np.float32)
    u = fe.dzi_draws_numpy(B, 99)
    assert u.dtype == np.float32 and u.min() >= -1 and u.max() < 1 and abs(u.mean()) < 0.1
    assert np.array_equal(u * 2.0 ** 23, np.rint(u * 2.0 ** 23))                             # multiples of 2^-23: 2 r - 1 is exact
    for kw in (dict(), dict(pad_ratio=1.3, scale_ratio=0.4, shift_ratio=0.15)):
        c, s = fe.dzi_boxes_numpy(box, (480, 640), train=True, seed=99, **kw)
        a = dict(pad_ratio=1.5, scale_ratio=0.25, shift_ratio=0.25)
        a.update(kw)
        tc, ts = fe._dzi_torch(torch.from_numpy(box), (480, 640), a["pad_ratio"], a["scale_ratio"], a["shift_ratio"], torch.from_numpy(u))
        assert np.array_equal(c, tc.numpy()) and np.array_equal(s, ts.numpy())
        assert (s == 640).any() and (s < 640).any()
        c2, s2 = fe.dzi_boxes_numpy(box, (480, 640), train=True, u=u, **kw)
        assert np.array_equal(c, c2) and np.array_equal(s, s2)
        c0, s0 = fe.dzi_boxes_numpy(box, (480, 640), train=False, **kw)
        tc, ts = fe.dzi_boxes(torch.from_numpy(box), (480, 640), train=False, **kw)
        assert np.array_equal(c0, tc.numpy()) and np.array_equal(s0, ts.numpy())
    assert not np.array_equal(fe.dzi_draws_numpy(B, 100), u)
