"""GPU: the crop augmentation (ops.augment_crops, csrc/gdm_augment.hip), the hash-drawn box jitter (dzi_boxes(jitter="hash")) and the
augment= / jitter= legs of frontend.make_inputs_from_boxes.  The kernels' results are fixed by the rule in include/gdm.h, which
frontend.augment_crops_numpy and frontend.dzi_boxes_numpy restate: every comparison here is on bits, none has a tolerance.

The rule's motion blur cannot reach the loader's `a <= 0` early return: the length is below(D, 15) + 1 >= 1 and max(|cos|, |sin|) >=
0.707, so a >= 1 (the loader's int(rand * 15) + 1 has the same floor).  test_frontend_augment_cpu.py calls motion_taps(0, 0) for it;
here the seeds are chosen to contain a 1 x 1 kernel (a = 1), a single-tap kernel, and a >= 25."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from geometric_aware_dense_matching_amd import frontend as fe, ops, synthetic  # noqa: E402

B, NB, HB, WB = 6, 2, 80, 96
ENABLE = np.array([1, 1, 0, 1, 1, 1], np.uint8)


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _conditions(draws, enable):
    """What a batch with these draws exercises, over the passes that are applied."""
    got = set()
    for b, d in enumerate(draws):
        if enable is not None and not enable[b]:
            continue
        if d["second"]:
            got.add("second")
        for p in d["passes"][:2 if d["second"] else 1]:
            for k in ("sharpen", "motion", "gauss", "extra"):
                got.add("%s %s" % (k, "on" if p[k] else "off"))
            if p["gauss"]:
                got.add("gauss %d" % p["gauss_k"])
            if p["motion"]:
                if p["a"] >= 25:
                    got.add("motion a>=25")
                if p["a"] == 1:
                    got.add("motion a=1")
                if len(p["taps"]) == 1:
                    got.add("motion one tap")
                assert p["a"] >= 1                                 # a = 0 cannot be drawn (see the module docstring)
            if p["halo"] >= 16:
                got.add("halo>=16")
            if p["sharpen"] and p["motion"] and p["gauss"]:
                got.add("all three")
    return got


WANTED = {"second", "sharpen on", "sharpen off", "motion on", "motion off", "gauss on", "gauss off", "extra on", "extra off", "gauss 3",
          "gauss 5", "motion a>=25", "motion a=1", "motion one tap", "halo>=16", "all three"}


SEEDS = (12, 1279)                                                # found by a greedy cover of WANTED over the seeds 0 .. 2999


@pytest.fixture(scope="module")
def seeds():
    got = set()
    for x in SEEDS:
        got |= _conditions(fe.augment_draws_numpy(B, x), ENABLE)
    assert got >= WANTED, sorted(WANTED - got)                     # the batches provably contain every case, before anything is compared
    return SEEDS


def _inputs(S, seed):
    rs = np.random.RandomState(seed)
    lv = rs.randint(0, 256, size=(B, 3, S, S))
    lv[:, :, : S // 2] = (lv[:, :, : S // 2] // 64) * 64 + 20       # half of it smooth enough that the blurs do not average to grey
    rgb = fe.aug_normalise(lv)
    depth = (rs.uniform(0.3, 2.0, size=(B, S, S)) * (rs.rand(B, S, S) > 0.4)).astype(np.float32)
    depth[0, 0, :4] = (np.nan, -1.0, 1e-7, 2e-6)
    mask = rs.choice(np.array([0, 0, 3, 255], np.uint8), size=(B, S, S))
    bank = (rs.randint(0, 256, size=(NB, HB, WB, 3)).astype(np.uint8), rs.uniform(0.5, 3.0, size=(NB, HB, WB)).astype(np.float32),
            rs.choice(np.array([0, 9, 255], np.uint8), size=(NB, HB, WB)))
    return rgb, depth, mask, bank


def _same_bits(got, want):
    g = got.cpu().numpy()
    return g.dtype == want.dtype and g.shape == want.shape and np.array_equal(g.view(np.uint32), want.view(np.uint32))


def _run(rgb, depth, mask, bank, enable, seed):
    return ops.augment_crops(_cuda(rgb), _cuda(depth), mask=_cuda(mask), background=None if bank is None else tuple(_cuda(a) for a in bank),
                             enable=_cuda(enable), seed=seed)


@pytest.mark.parametrize("S", [32, 40, 72])
def test_kernel_equals_the_restatement(S, seeds):
    rgb, depth, mask, bank = _inputs(S, S)
    for seed in seeds:
        want = fe.augment_crops_numpy(rgb, depth, mask, bank, ENABLE, seed)
        got = _run(rgb, depth, mask, bank, ENABLE, seed)
        assert _same_bits(got[0], want[0]), (S, seed, "rgb")
        assert _same_bits(got[1], want[1]), (S, seed, "depth")
        assert np.array_equal(want[0][2].view(np.uint32), rgb[2].view(np.uint32)) and not np.array_equal(want[0][0], rgb[0])
        # no background: the depth comes back as it went in; no enable: crop 2 is augmented too
        want = fe.augment_crops_numpy(rgb, depth, None, None, None, seed)
        got = _run(rgb, depth, None, None, None, seed)
        assert _same_bits(got[0], want[0]) and _same_bits(got[1], depth), (S, seed, "no background")
        assert not np.array_equal(want[0][2], rgb[2])
        want = fe.augment_crops_numpy(rgb, depth, mask, bank, None, seed)
        got = _run(rgb, depth, mask, bank, None, seed)
        assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), (S, seed, "no enable")


def test_device_seed_word_and_repeatability(seeds):
    rgb, depth, mask, bank = _inputs(40, 1)
    seed = seeds[0]
    a = _run(rgb, depth, mask, bank, ENABLE, seed)
    b = _run(rgb, depth, mask, bank, ENABLE, seed)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    word = torch.tensor([seed], dtype=torch.int32, device="cuda")
    c = _run(rgb, depth, mask, bank, ENABLE, word)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    big = 0xfedcba98                                               # a word with the top bit set, as an int and as int32 on the device
    d = _run(rgb, depth, mask, bank, ENABLE, big)
    e = _run(rgb, depth, mask, bank, ENABLE, torch.tensor([big - (1 << 32)], dtype=torch.int32, device="cuda"))
    assert torch.equal(d[0], e[0]) and torch.equal(d[1], e[1]) and not torch.equal(a[0], d[0])
    want = fe.augment_crops_numpy(rgb, depth, mask, bank, ENABLE, big)
    assert _same_bits(d[0], want[0]) and _same_bits(d[1], want[1])


def test_arguments_are_checked():
    rgb, depth, mask, bank = _inputs(32, 2)
    with pytest.raises(ValueError):
        _run(rgb[:, :, :31, :31], depth[:, :31, :31], None, None, None, 0)
    with pytest.raises(ValueError):
        _run(rgb, depth, None, bank, None, 0)
    with pytest.raises(ValueError):
        _run(rgb, depth, mask, tuple(a[:, :33] for a in bank), None, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.augment_crops(torch.from_numpy(rgb), torch.from_numpy(depth))


def test_dzi_boxes_hash_equals_the_restatement():
    rs = np.random.RandomState(3)
    n = 301
    x1, y1 = rs.uniform(0, 400, n), rs.uniform(0, 300, n)
    box = np.stack([x1, y1, x1 + rs.uniform(5, 600, n), y1 + rs.uniform(5, 600, n)], axis=1).astype(np.float32)
    for train in (True, False):
        for kw in (dict(), dict(pad_ratio=1.3, scale_ratio=0.4, shift_ratio=0.15)):
            c, s = fe.dzi_boxes(_cuda(box), (480, 640), train=train, jitter="hash", seed=77, **kw)
            wc, ws = fe.dzi_boxes_numpy(box, (480, 640), train=train, seed=77, **kw)
            assert _same_bits(c, wc) and _same_bits(s, ws), (train, kw)
    word = torch.tensor([77], dtype=torch.int32, device="cuda")
    c2, s2 = fe.dzi_boxes(_cuda(box), (480, 640), train=True, jitter="hash", seed=word)
    wc, ws = fe.dzi_boxes_numpy(box, (480, 640), train=True, seed=77)
    assert _same_bits(c2, wc) and _same_bits(s2, ws)
    c3, _ = fe.dzi_boxes(_cuda(box), (480, 640), train=True, jitter="hash", seed=78)
    assert not torch.equal(c3, c2)
    g = torch.Generator(device="cuda").manual_seed(1)
    old = fe.dzi_boxes(_cuda(box), (480, 640), train=True, generator=g)
    g = torch.Generator(device="cuda").manual_seed(1)
    new = fe.dzi_boxes(_cuda(box), (480, 640), train=True, generator=g, jitter="torch", seed=5)
    assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1])


H, W, S_ITEM, N_ITEM = 480, 640, 64, 256


def _frames(seed, n):
    rs = np.random.RandomState(seed)
    fr = [synthetic.make_frame(rs) for _ in range(n)]
    det = [synthetic.make_box_mask(rs) for _ in range(n)]
    K = np.stack([synthetic.LM_K * np.float32(1.0 + 0.07 * b) for b in range(n)]).astype(np.float32)
    K[:, 2, 2] = 1.0
    return dict(rgb_u8=np.stack([f[1] for f in fr]), depth=np.stack([f[0] for f in fr]), K=K,
                bbox_xyxy=np.stack([d[0] for d in det]), mask=np.stack([d[1] for d in det]))


def _bank(seed):
    rs = np.random.RandomState(seed)
    return (rs.randint(0, 256, size=(NB, HB, WB, 3)).astype(np.uint8), rs.uniform(0.5, 1.5, size=(NB, HB, WB)).astype(np.float32),
            rs.choice(np.array([0, 9, 255], np.uint8), size=(NB, HB, WB)))


@pytest.mark.parametrize("depth_fill", ["fast", "multiscale"])
def test_make_inputs_from_boxes_augmented_item(depth_fill):
    n, seed = 3, 31
    fr, bank = _frames(91, n), _bank(92)
    d = {k: _cuda(v) for k, v in fr.items()}
    dbank = tuple(_cuda(a) for a in bank)
    enable = np.array([1, 0, 1], np.uint8)
    args = (d["rgb_u8"], d["depth"], d["K"], d["bbox_xyxy"], S_ITEM, N_ITEM)
    inp = fe.make_inputs_from_boxes(*args, mask=d["mask"], train=True, depth_fill=depth_fill, sampler="hash", jitter="hash", seed=seed,
                                    augment=dict(background=dbank, enable=_cuda(enable)), build_pyramid=False)
    # the chain of the restatements: box jitter -> crop -> augmentation; then the device's own fill (its last stage multiplies by expf,
    # whose last bit differs from numpy's, test_gpu_frontend_fill.py) -> normals, points and assembly restated on that filled crop
    center, scale = fe.dzi_boxes_numpy(fr["bbox_xyxy"], (H, W), train=True, seed=seed)
    assert _same_bits(inp["center"], center) and _same_bits(inp["scale"], scale)
    crop = fe.crop_from_boxes_numpy(fr["rgb_u8"], fr["depth"], np.zeros((n, 3, H, W), np.float32), fr["K"], center, scale, S_ITEM,
                                    mask=fr["mask"])
    rgb, dep = fe.augment_crops_numpy(crop["rgb"], crop["depth"], crop["mask"], bank, enable, seed)
    assert _same_bits(inp["rgb"], rgb) and _same_bits(inp["depth_aug"], dep)
    assert np.array_equal(rgb[1], crop["rgb"][1]) and not np.array_equal(rgb[0], crop["rgb"][0]) and not np.array_equal(dep[0], crop["depth"][0])
    assert _same_bits(inp["dpt_xyz"], crop["dpt_xyz"])                                       # untouched, as in the reference
    filled = fe.fill_depth(_cuda(dep), mode=depth_fill)
    assert torch.equal(inp["depth_filled"], filled)
    vd = filled.cpu().numpy()
    want = fe.sample_assemble_numpy(vd, crop["dpt_xyz"], rgb, fe.depth_normals_numpy(vd, fr["K"]), crop["mask"], N_ITEM, seed)
    assert np.array_equal(inp["choose"][:, 0].cpu().numpy(), want[0]) and np.array_equal(inp["cld_rgb_nrm"].cpu().numpy(), want[1])
    assert np.array_equal(inp["origin_labels"].cpu().numpy(), want[2]) and np.array_equal(inp["n_valid"].cpu().numpy(), want[3])
    # augment=None, jitter="torch" is today's call, key for key
    g = torch.Generator(device="cuda").manual_seed(5)
    old = fe.make_inputs_from_boxes(*args, mask=d["mask"], train=True, depth_fill=depth_fill, generator=g, sampler="hash", seed=seed,
                                    build_pyramid=False)
    g = torch.Generator(device="cuda").manual_seed(5)
    new = fe.make_inputs_from_boxes(*args, mask=d["mask"], train=True, depth_fill=depth_fill, generator=g, sampler="hash", seed=seed,
                                    build_pyramid=False, augment=None, jitter="torch")
    assert sorted(old) == sorted(new) and "depth_aug" not in old and all(torch.equal(old[k], new[k]) for k in old)
    assert sorted(inp) == sorted(list(old) + ["depth_aug"])
    with pytest.raises(ValueError):
        fe.make_inputs_from_boxes(*args, mask=d["mask"], augment=dict(background=None))      # no depth_fill: the LineMOD item has none
    with pytest.raises(ValueError):
        fe.make_inputs_from_boxes(*args, depth_fill=depth_fill, augment=dict(background=None))           # no mask


def test_augmented_item_captures_and_redraws_per_replay():
    n = 3
    fr, bank = _frames(93, n), _bank(94)
    d = {k: _cuda(v) for k, v in fr.items()}
    aug = dict(background=tuple(_cuda(a) for a in bank), enable=None)
    word = torch.zeros(1, dtype=torch.int32, device="cuda")

    def item(seed):
        return fe.make_inputs_from_boxes(d["rgb_u8"], d["depth"], d["K"], d["bbox_xyxy"], S_ITEM, N_ITEM, mask=d["mask"], train=True,
                                         depth_fill="multiscale", sampler="hash", jitter="hash", seed=seed, augment=aug,
                                         build_pyramid=False)

    words = (7, 8, -1234567)
    eager = [{k: v.clone() for k, v in item(w & 0xffffffff).items()} for w in words]
    assert not torch.equal(eager[0]["rgb"], eager[1]["rgb"]) and not torch.equal(eager[0]["center"], eager[1]["center"])
    pool = ops.BufferPool()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), ops.buffer_pool(pool):
        for _ in range(2):
            item(word)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), ops.buffer_pool(pool):
        out = item(word)
    for w, ref in zip(words, eager):
        word.fill_(w)
        g.replay()
        torch.cuda.synchronize()
        assert sorted(out) == sorted(ref)
        for k in ref:
            assert torch.equal(out[k], ref[k]), (w, k)
