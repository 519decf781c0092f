"""CPU: the static bookkeeping of the edge-grouped SplineConv (splinecnn.build_spline_pairs) -- the inverse maps the training path
(`SplineCNN_Mesh.train_path = "grouped"`) gathers through are exact inverses of `pos` / `rowidx` -- and the command-line flag."""
import numpy as np
import pytest
import torch

from geometric_aware_dense_matching_amd import splinecnn


def hand_made_csr():
    """A 10-vertex graph in CSR (target-sorted) form with a degree-0 vertex (0), a degree-7 vertex (1), two identical edges into
    vertex 2 (same source, same pseudo-coordinates: a pair shared by several edges) and pseudo-coordinates of exactly 0.0 and 1.0
    (zero-basis corners, wrapped kernel indices).  -> rowptr i32[M+1], src i32[E], attr f32[E,3], M."""
    edges = {1: [2, 3, 4, 5, 6, 7, 8], 2: [3, 3], 3: [0, 9], 4: [1], 5: [1, 4], 6: [9], 7: [0, 1, 2], 8: [7], 9: [8, 3]}
    M = 10
    rs = np.random.RandomState(11)
    rowptr, src, attr = [0], [], []
    for i in range(M):
        for j in edges.get(i, []):
            src.append(j)
            attr.append(rs.rand(3))
        rowptr.append(len(src))
    attr = np.asarray(attr, dtype=np.float32)
    attr[2] = attr[3] = (0.25, 0.5, 0.8125)         # lattice points in two dimensions: six of the eight corners have zero basis
    attr[7] = attr[8]                               # the two identical edges 3 -> 2
    attr[0] = (0.0, 1.0, 0.3)
    attr[-1] = (1.0, 1.0, 1.0)
    return (torch.tensor(rowptr, dtype=torch.int32), torch.tensor(src, dtype=torch.int32), torch.from_numpy(attr), M)


def random_csr(M, seed):
    """k = 4 random sources per vertex (no kNN kernel on the CPU), a few coordinates on the lattice."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, M, (4 * M,), generator=g).to(torch.int32)
    attr = torch.rand(4 * M, 3, generator=g)
    attr[::7, 0] = 0.0
    attr[3::11, 2] = 1.0
    rowptr = (torch.arange(M + 1) * 4).to(torch.int32)
    return rowptr, src, attr, M


def check_inverse_maps(pairs, rowptr, src, M):
    """The properties the gather-form backward rests on; shared with the GPU tests (which run them on the device-built maps)."""
    E = src.shape[0]
    p = {k: v.cpu() for k, v in pairs.items()}
    R = p["rowidx"].shape[0]
    pos = p["pos"].long().reshape(-1)
    # pair -> (edge, corner): every (edge, corner) exactly once, in ascending order inside a row, and listed under ITS row
    assert p["pair_ptr"].shape == (R + 1,) and p["pair_ec"].shape == (8 * E,) and p["pair_ptr"].dtype == p["pair_ec"].dtype == torch.int32
    assert int(p["pair_ptr"][0]) == 0 and int(p["pair_ptr"][-1]) == 8 * E
    assert torch.equal(torch.sort(p["pair_ec"].long())[0], torch.arange(8 * E))
    counts = (p["pair_ptr"][1:] - p["pair_ptr"][:-1]).long()
    assert bool((counts >= 0).all())
    owner = torch.repeat_interleave(torch.arange(R), counts)
    assert torch.equal(pos[p["pair_ec"].long()], owner)
    same_row = owner[1:] == owner[:-1]
    assert bool((p["pair_ec"][1:][same_row] > p["pair_ec"][:-1][same_row]).all())
    # blocks: padding excluded, real rows contiguous from blk_start, kernel index = tile_co0 / cout of the row's tile
    start, rows = p["blk_start"].long(), p["blk_rows"].long()
    assert start.shape == rows.shape == (125,)
    real = torch.zeros(R, dtype=torch.bool)
    for k in range(125):
        real[start[k]: start[k] + rows[k]] = True
        if rows[k] > 0:
            assert start[k] % 256 == 0 and bool((p["tile_co0"][start[k] // 256: (start[k] + rows[k] + 255) // 256] == 128 * k).all())
    U = int(real.sum())
    assert int(rows.sum()) == U == torch.unique(pos).shape[0]
    assert torch.equal(counts > 0, real)                                   # padding rows are in no list, every real row is in use
    # source -> pair rows: real rows only, each exactly once, ascending per source, and under ITS source
    assert p["src_ptr"].shape == (M + 1,) and p["src_rows"].shape == (U,)
    assert int(p["src_ptr"][0]) == 0 and int(p["src_ptr"][-1]) == U
    assert torch.equal(torch.sort(p["src_rows"].long())[0], torch.nonzero(real).reshape(-1))
    scount = (p["src_ptr"][1:] - p["src_ptr"][:-1]).long()
    sowner = torch.repeat_interleave(torch.arange(M), scount)
    assert torch.equal(p["rowidx"].long()[p["src_rows"].long()], sowner)
    same_src = sowner[1:] == sowner[:-1]
    assert bool((p["src_rows"][1:][same_src] > p["src_rows"][:-1][same_src]).all())
    # every edge's eight pairs have the edge's source
    assert torch.equal(p["rowidx"].long()[p["pos"].long()], src.long().cpu()[:, None].expand(E, 8))
    assert torch.equal(p["rowid"].long(), torch.arange(R))
    # target side
    deg = (rowptr[1:] - rowptr[:-1]).long().cpu()
    assert torch.equal(p["tgt"].long(), torch.repeat_interleave(torch.arange(M), deg))
    assert p["inv_deg"].dtype == torch.float32 and p["inv_deg"].shape == (M,)
    assert torch.equal(p["inv_deg"], torch.where(deg > 0, 1.0 / deg.clamp(min=1).float(), torch.zeros(())))
    return U


@pytest.mark.parametrize("case", ["random40", "hand_made"])
def test_inverse_maps_are_exact_inverses(case):
    rowptr, src, attr, M = random_csr(40, 2) if case == "random40" else hand_made_csr()
    old = splinecnn.build_spline_pairs(src, attr, M)
    pairs = splinecnn.build_spline_pairs(src, attr, M, rowptr=rowptr)
    U = check_inverse_maps(pairs, rowptr, src, M)
    for k in ("rowidx", "tile_co0", "pos", "basis"):                     # the existing keys keep their values
        assert torch.equal(old[k], pairs[k]), k
    if case == "hand_made":
        deg = rowptr[1:] - rowptr[:-1]
        assert int(deg[0]) == 0 and int(deg[1]) == 7 and float(pairs["inv_deg"][0]) == 0.0
        assert torch.equal(pairs["pos"][7], pairs["pos"][8])               # the identical edges share all eight pairs
        assert U < 8 * src.shape[0]
        assert int((pairs["basis"] == 0).sum()) >= 4                       # zero-basis corners exist
        assert int((pairs["blk_rows"] == 0).sum()) > 0                     # and empty kernel indices


def test_mesh_train_path_flag():
    from geometric_aware_dense_matching_amd import train_lm, train_ycb
    from geometric_aware_dense_matching_amd.splinecnn import SplineCNN_Mesh
    assert SplineCNN_Mesh.train_path == "dense"
    for mod in (train_lm, train_ycb):
        assert mod.build_parser().parse_args([]).mesh_train_path == "dense"
        assert mod.build_parser().parse_args("--mesh-train-path grouped".split()).mesh_train_path == "grouped"
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args("--mesh-train-path table".split())
    a = train_lm.build_parser().parse_args("-cls_id=1 --n-mesh 64 --n-points 256 --mesh-train-path grouped".split())
    grouped = train_lm.build_model(a, 1)
    a.mesh_train_path = "dense"
    dense = train_lm.build_model(a, 1)
    assert grouped.model_emb.train_path == "grouped" and dense.model_emb.train_path == "dense"
    assert "train_path" not in grouped.model_emb.__dict__ or SplineCNN_Mesh.train_path == "dense"    # the class default is untouched
    assert list(grouped.state_dict()) == list(dense.state_dict())
    grouped.model_emb.train_path = "table"
    with pytest.raises(ValueError, match="train_path"):
        grouped.model_emb()
