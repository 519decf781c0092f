"""CPU: the hash-sampling rule of include/gdm.h (gdm_sample_assemble_hip) as frontend.sample_assemble_numpy restates it -- the
properties the definition promises, on small maps built directly so that the valid counts are exact -- and the library that holds
the kernel cross-compiles for gfx950 and refuses bad arguments before any HIP call."""
import ctypes
import os

import numpy as np
import pytest

from geometric_aware_dense_matching_amd import frontend, pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _maps(B, S, n_valid, seed=0, with_mask=True):
    """Crops with exactly n_valid[b] valid pixels at random places; the invalid ones are 0, negative or NaN."""
    rs = np.random.RandomState(seed)
    P = S * S
    vd = np.zeros((B, P), np.float32)
    for b in range(B):
        bad = rs.choice(np.array([0.0, -0.7, np.nan, 1e-7], np.float32), size=P)
        vd[b] = bad
        vd[b, rs.permutation(P)[:n_valid[b]]] = rs.uniform(0.3, 2.0, size=n_valid[b]).astype(np.float32)
    xyz = rs.randn(B, S, S, 3).astype(np.float32)
    rgb = rs.randn(B, 3, S, S).astype(np.float32)
    nrm = rs.randn(B, 3, S, S).astype(np.float32)
    mask = rs.choice(np.array([0, 255, 3], np.uint8), size=(B, S, S)) if with_mask else None
    return vd.reshape(B, S, S), xyz, rgb, nrm, mask


def test_mixer_is_the_ransac_samplers():
    x = np.arange(0, 1 << 20, 997, dtype=np.uint32)
    with np.errstate(over="ignore"):
        assert np.array_equal(frontend._mix32(x), pose._mix32(x))
    # by hand: key of crop 1, pixel 5, seed 7
    def mix(v):
        v ^= v >> 16
        v = (v * 0x7feb352d) & 0xffffffff
        v ^= v >> 15
        v = (v * 0x846ca68b) & 0xffffffff
        return v ^ (v >> 16)
    assert int(frontend.sample_keys(2, 8, seed=7)[1, 5]) == mix(mix(mix(7 ^ 0x9e3779b9) ^ 1) ^ 5)


def test_keys_are_pairwise_distinct_for_a_whole_crop():
    for seed in (0, 1, 0xdeadbeef):
        keys = frontend.sample_keys(3, 65536, seed)
        for b in range(3):
            assert len(np.unique(keys[b])) == 65536


def test_subset_when_enough_valid_pixels():
    S, N = 32, 200
    nv = [200, 201, 600, 1024]
    vd, xyz, rgb, nrm, mask = _maps(4, S, nv)
    choose, cld, labels, n_valid = frontend.sample_assemble_numpy(vd, xyz, rgb, nrm, mask, N, seed=3)
    assert choose.dtype == np.int32 and choose.shape == (4, N) and n_valid.dtype == np.int32 and n_valid.tolist() == nv
    flat = vd.reshape(4, -1)
    for b in range(4):
        assert len(np.unique(choose[b])) == N
        assert (flat[b, choose[b]] > np.float32(1e-6)).all()
        keys = frontend.sample_keys(4, S * S, 3)[b]
        assert (np.diff(keys[choose[b]].astype(np.int64)) > 0).all()                    # ascending key
        valid = np.nonzero(flat[b] > np.float32(1e-6))[0]
        assert keys[choose[b]].max() == np.sort(keys[valid])[N - 1]                      # the N smallest keys, no other


def test_wrap_around_and_empty_crops():
    S, N = 16, 100
    nv = [0, 1, 37, 99]
    vd, xyz, rgb, nrm, mask = _maps(4, S, nv, seed=5)
    choose, cld, labels, n_valid = frontend.sample_assemble_numpy(vd, xyz, rgb, nrm, mask, N, seed=11)
    assert n_valid.tolist() == nv
    assert not choose[0].any()                                                           # choose = [0]
    flat = vd.reshape(4, -1)
    for b in (1, 2, 3):
        valid = np.nonzero(flat[b] > np.float32(1e-6))[0]
        assert np.array_equal(np.sort(choose[b, :nv[b]]), valid)                         # a permutation of the valid set
        assert np.array_equal(choose[b], choose[b, np.arange(N) % nv[b]])
    # gathers at pixel 0 for the empty crop
    assert np.array_equal(cld[0, :3], np.repeat(xyz[0].reshape(-1, 3)[0][:, None], N, axis=1))


def test_seed_and_crop_index_decide_the_order():
    S, N = 32, 300
    vd, xyz, rgb, nrm, mask = _maps(1, S, [700], seed=2)
    two = [np.repeat(a, 2, axis=0) for a in (vd, xyz, rgb, nrm, mask)]                   # the same crop as b = 0 and b = 1
    a = frontend.sample_assemble_numpy(*two, N, seed=4)
    b = frontend.sample_assemble_numpy(*two, N, seed=4)
    c = frontend.sample_assemble_numpy(*two, N, seed=5)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert not np.array_equal(a[0], c[0])
    assert not np.array_equal(a[0][0], a[0][1])
    assert np.array_equal(a[3], c[3])
    # the seed is a 32-bit word
    d = frontend.sample_assemble_numpy(*two, N, seed=4 + (1 << 32))
    assert np.array_equal(a[0], d[0])


def test_assembly_is_the_plain_gathers():
    S, N = 24, 150
    vd, xyz, rgb, nrm, mask = _maps(3, S, [10, 150, 500], seed=8)
    choose, cld, labels, _ = frontend.sample_assemble_numpy(vd, xyz, rgb, nrm, mask, N, seed=1)
    assert cld.dtype == np.float32 and cld.shape == (3, 9, N) and labels.dtype == np.uint8
    for b in range(3):
        ch = choose[b]
        want = np.concatenate([xyz[b].reshape(-1, 3)[ch].T, rgb[b].reshape(3, -1)[:, ch], nrm[b].reshape(3, -1)[:, ch]], axis=0)
        assert np.array_equal(cld[b], want)
        lab = mask[b].reshape(-1)[ch]
        assert np.array_equal(labels[b], np.where(lab == 255, 1, lab))
    assert set(np.unique(labels)) == {0, 1, 3}
    assert frontend.sample_assemble_numpy(vd, xyz, rgb, nrm, None, N, seed=1)[2] is None


def test_inclusion_counts_are_binomial():
    """N = 2048 of 65 536 valid pixels over 200 seeds: every pixel is included with probability 1/32 per seed, so the inclusion
    counts have mean 6.25 and the binomial variance 200 / 32 * 31 / 32 = 6.0547; measured within 10 % of it."""
    P, N, seeds = 65536, 2048, 200
    counts = np.zeros(P, np.int64)
    for seed in range(seeds):
        keys = frontend.sample_keys(1, P, seed)[0]
        counts[np.argpartition(keys, N - 1)[:N]] += 1
    assert counts.sum() == seeds * N
    want = seeds * (N / P) * (1 - N / P)
    print("inclusion counts: mean %.4f variance %.4f (binomial %.4f)" % (counts.mean(), counts.var(), want))
    assert abs(counts.var() - want) < 0.1 * want


def test_library_cross_compiles_and_refuses_bad_arguments():
    from geometric_aware_dense_matching_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.lib()
    assert b"gfx950" in open(_lib.LIB_PATH, "rb").read()
    assert b"sample_assemble_kernel" in open(_lib.LIB_PATH, "rb").read()
    hdr = open(os.path.join(ROOT, "include", "gdm.h")).read()
    assert "#define GDM_SAMPLE_MAX_N %d" % _lib.GDM_SAMPLE_MAX_N in hdr and _lib.GDM_SAMPLE_MAX_N >= 4096
    assert "#define GDM_SAMPLE_MAX_S %d" % _lib.GDM_SAMPLE_MAX_S in hdr
    assert lib.gdm_sample_assemble_workspace_bytes(16, 256) == 16 * 65536 // 8
    assert lib.gdm_sample_assemble_workspace_bytes(1, 37) == ((37 * 37 + 63) // 64) * 8
    assert lib.gdm_sample_assemble_workspace_bytes(0, 256) == 0
    assert lib.gdm_sample_assemble_workspace_bytes(1, _lib.GDM_SAMPLE_MAX_S + 1) == 0
    buf = (ctypes.c_char * 65536)()
    p = ctypes.addressof(buf)

    def call(B=1, S=8, N=16, ws=65536, vd=p, mask=None, labels=None):
        return lib.gdm_sample_assemble_hip(vd, p, p, p, mask, B, S, N, 0, None, p, p, labels, p, p, ws, None)

    for kw, msg in ((dict(vd=None), b"NULL"), (dict(mask=p), b"mask and labels"), (dict(labels=p), b"mask and labels"),
                    (dict(B=0), b"B=0"), (dict(S=0), b"S=0"), (dict(N=0), b"N=0"), (dict(N=-3), b"N=-3"),
                    (dict(N=_lib.GDM_SAMPLE_MAX_N + 1), b"N=4097"), (dict(S=_lib.GDM_SAMPLE_MAX_S + 1), b"S=4097"),
                    (dict(S=256, ws=8191), b"workspace")):
        assert call(**kw) == -1, kw
        assert msg in lib.gdm_last_error(), (kw, lib.gdm_last_error())


def test_ops_and_frontend_refuse_what_they_cannot_do():
    import torch
    from geometric_aware_dense_matching_amd import ops
    z = torch.zeros(1, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_assemble(z, torch.zeros(1, 4, 4, 3), torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), 8)
    with pytest.raises(ValueError, match="sampler"):
        frontend.make_inputs_from_boxes(None, z, None, None, 4, 8, sampler="sobol")
