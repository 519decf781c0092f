"""tests/stream_audit.py on synthetic logs built by hand: the vector clocks, both rules, the decoding of job structures and the
recorder, without a GPU.  No race is staged on a device anywhere: a bad ordering exists only as a log."""
import ctypes
import io
import os
import tokenize

import pytest
import torch

import stream_audit as sa
from geometric_aware_dense_matching_amd import _lib

MAIN, SIDE, SIDE2 = "main", "side0", "side2"
X, Y, P = 0x1000, 0x2000, 0x3000          # storages ("addresses")


def _r1(log):
    rep = sa.analyse(log, exceptions={})
    return rep, [(v.what, v.first[0], v.second[0]) for v in rep.r1]


def _fork_use_join(join=True, record_streams=True):
    """main writes x; the side stream (forked behind main) reads x and writes y; main joins and reads y.  x and y are allocated
    during the step, on the stream that writes them."""
    log = [sa.alloc(X, MAIN), sa.access(MAIN, "make_x", writes=[(X, 0, 64, "x")])]
    log += sa.wait_stream(SIDE, MAIN, site=("fork",))
    if record_streams:
        log.append(sa.keep(X, SIDE, site=("use",)))
    log += [sa.alloc(Y, SIDE), sa.access(SIDE, "body", reads=[(X, 0, 64, "x")], writes=[(Y, 0, 64, "y")])]
    if join:
        log += sa.wait_stream(MAIN, SIDE, site=("join",))
    if record_streams:
        log.append(sa.keep(Y, MAIN, site=("join-keep",)))
    log.append(sa.access(MAIN, "consume", reads=[(Y, 0, 64, "y")]))
    return log


def test_correct_fork_use_join_passes():
    rep = sa.analyse(_fork_use_join(), exceptions={})
    assert not rep.violations and not rep.unresolved
    assert rep.streams == {MAIN, SIDE} and rep.accesses == 3
    assert rep.ordered == {(MAIN, SIDE), (SIDE, MAIN)}          # both hand-overs are seen as ordered write-then-read pairs


def test_missing_join_fails_r1():
    rep, bad = _r1(_fork_use_join(join=False))
    assert bad == [("write-then-read", "body", "consume")]
    v = rep.r1[0]
    assert v.first[1] == SIDE and v.second[1] == MAIN and v.first[3] == "y" and "body" in str(v) and "consume" in str(v)


def test_missing_fork_wait_fails_r1():
    log = [e for e in _fork_use_join() if not (e.kind == "sync" and e.site == ("fork",))]
    assert _r1(log)[1] == [("write-then-read", "make_x", "body")]


def test_write_after_read_needs_the_consumers_event():
    """The producer hands x to the consumer with an event; the consumer reads; the producer then overwrites x in place without
    waiting for the consumer.  The producer-to-consumer event does not order that."""
    log = [sa.access(MAIN, "produce", writes=[(P, 0, 64, "x")]), sa.record(MAIN, "e1"), sa.wait(SIDE, "e1"),
           sa.access(SIDE, "consume", reads=[(P, 0, 64, "x")]),
           sa.access(MAIN, "overwrite", writes=[(P, 0, 64, "x")])]
    assert _r1(log)[1] == [("read-then-write", "consume", "overwrite")]
    fixed = log[:-1] + [sa.record(SIDE, "e2"), sa.wait(MAIN, "e2"), log[-1]]
    assert not _r1(fixed)[1]


def test_write_after_write_on_two_streams():
    log = [sa.access(MAIN, "a", writes=[(P, 0, 64, "x")]), sa.access(SIDE, "b", writes=[(P, 32, 96, "x")])]
    assert _r1(log)[1] == [("write-then-write", "a", "b")]


def test_cloud_only_wait_does_not_cover_what_is_written_after_it():
    """pyramid.wait_ready(cloud_only=True): the waiter holds READY_CLOUD's snapshot; an index written behind that record is not
    ordered for it until it waits for READY."""
    log = [sa.access(SIDE2, "knn_first", writes=[(X, 0, 64, "cld_nei_idx0")]), sa.record(SIDE2, "READY_CLOUD"),
           sa.access(SIDE2, "knn_rest", writes=[(Y, 0, 64, "r2p_ds_nei_idx0")]), sa.record(SIDE2, "READY"),
           sa.wait(SIDE, "READY_CLOUD"),
           sa.access(SIDE, "lfa", reads=[(X, 0, 64, "cld_nei_idx0")]),
           sa.access(SIDE, "fuse", reads=[(Y, 0, 64, "r2p_ds_nei_idx0")])]
    rep, bad = _r1(log)
    assert bad == [("write-then-read", "knn_rest", "fuse")] and rep.r1[0].second[3] == "r2p_ds_nei_idx0"
    assert not _r1(log[:-1] + [sa.wait(SIDE, "READY"), log[-1]])[1]


def test_a_rerecorded_event_carries_its_latest_record():
    w1, w2 = sa.access(MAIN, "w1", writes=[(X, 0, 64, "a")]), sa.access(MAIN, "w2", writes=[(Y, 0, 64, "b")])
    read_b = sa.access(SIDE, "r", reads=[(Y, 0, 64, "b")])
    # recorded again behind w2: the wait covers w2
    assert not _r1([w1, sa.record(MAIN, "e"), w2, sa.record(MAIN, "e"), sa.wait(SIDE, "e"), read_b])[1]
    # recorded once, in front of w2: it does not
    assert _r1([w1, sa.record(MAIN, "e"), w2, sa.wait(SIDE, "e"), read_b])[1] == [("write-then-read", "w2", "r")]
    # the waiter keeps what it waited for when the event is recorded again afterwards, and gains nothing from the new record
    log = [w1, sa.record(MAIN, "e"), sa.wait(SIDE, "e"), w2, sa.record(MAIN, "e"), sa.access(SIDE, "ra", reads=[(X, 0, 64, "a")]), read_b]
    assert _r1(log)[1] == [("write-then-read", "w2", "r")]
    # an event that was never recorded orders nothing
    assert _r1([w2, sa.wait(SIDE, "never"), read_b])[1] == [("write-then-read", "w2", "r")]


def test_overlapping_and_disjoint_views_of_one_storage():
    w = sa.access(MAIN, "w", writes=[(P, 0, 64, "rows 0-15")])
    assert not _r1([w, sa.access(SIDE, "r", reads=[(P, 64, 128, "rows 16-31")])])[1]          # [0,64) and [64,128) only touch
    assert _r1([w, sa.access(SIDE, "r", reads=[(P, 63, 128, "rows 15-31")])])[1] == [("write-then-read", "w", "r")]
    assert not _r1([sa.access(MAIN, "r1", reads=[(P, 0, 64, "x")]), sa.access(SIDE, "r2", reads=[(P, 0, 64, "x")])])[1]      # two reads


def test_missing_record_stream_fails_r2_and_persistent_buffers_are_exempt():
    rep = sa.analyse(_fork_use_join(record_streams=False), exceptions={})
    assert not rep.r1
    got = sorted((v.what, v.first[0], v.second[0], v.second[3]) for v in rep.r2)
    assert got == [("no record_stream(main)", "alloc", "consume", "y"), ("no record_stream(side0)", "alloc", "body", "x")]
    # record_stream on the wrong stream does not count
    log = _fork_use_join(record_streams=False) + [sa.keep(X, MAIN), sa.keep(Y, SIDE)]
    assert len(sa.analyse(log, exceptions={}).r2) == 2
    # the same accesses on buffers that existed before the step (no alloc entry): exempt from R2 ...
    persistent = [e for e in _fork_use_join(record_streams=False) if e.kind != "alloc"]
    assert not sa.analyse(persistent, exceptions={}).violations
    # ... and still under R1
    assert _r1([e for e in persistent if not (e.kind == "sync" and e.site == ("join",))])[1] == [("write-then-read", "body", "consume")]


def test_synchronize_orders_everything():
    w = [sa.access(MAIN, "w", writes=[(X, 0, 64, "a")]), sa.access(SIDE, "v", writes=[(Y, 0, 64, "b")])]
    r = [sa.access(SIDE2, "r", reads=[(X, 0, 64, "a"), (Y, 0, 64, "b")])]
    assert len(_r1(w + r)[1]) == 2
    assert not _r1(w + [sa.synchronize()] + r)[1]                                            # torch.cuda.synchronize
    assert _r1(w + [sa.synchronize(stream=MAIN)] + r)[1] == [("write-then-read", "v", "r")]     # Stream.synchronize: that stream only
    assert _r1(w + [sa.record(SIDE, "e"), sa.synchronize(event="e")] + r)[1] == [("write-then-read", "w", "r")]     # Event.synchronize
    # what is enqueued behind the synchronize is not covered by it
    late = sa.access(MAIN, "late", writes=[(X, 0, 64, "a")])
    assert _r1(w + [sa.synchronize(), late] + r)[1] == [("write-then-read", "late", "r")]
    # an event recorded behind a synchronize carries what the host waited for
    log = w + [sa.synchronize(), sa.record(SIDE2, "e"), sa.wait(MAIN, "e"), sa.access(MAIN, "again", writes=[(Y, 0, 64, "b")])]
    assert not _r1(log)[1]


def test_exceptions_are_keyed_by_entry_and_role_and_reported():
    log = _fork_use_join(join=False)
    rep = sa.analyse(log, exceptions={("consume", "y"): "a written reason"})
    assert not rep.r1 and len(rep.excepted) == 1 and rep.used_exceptions == {("consume", "y")}
    assert sa.analyse(log, exceptions={("consume", "x"): "another tensor"}).r1
    assert sa.EXCEPTIONS == {} or all(isinstance(k, tuple) and len(k) == 2 and why for k, why in sa.EXCEPTIONS.items())


def test_sensitivity_helpers_remove_one_call_site():
    log = _fork_use_join()
    assert sa.sites(log, "wait") == [("fork",), ("join",)] and sa.sites(log, "keep") == [("use",), ("join-keep",)]
    for site in sa.sites(log, "wait"):
        assert sa.analyse(sa.without(log, "wait", site), exceptions={}).r1, site
    for site in sa.sites(log, "keep"):
        rep = sa.analyse(sa.without(log, "keep", site), exceptions={})
        assert rep.r2 and not rep.r1, site
    assert sa.sequence(log)[:3] == [("make_x", "main"), ("wait_stream:record", "main"), ("wait_stream:wait", "side0")]


# ---- the package's ordering calls ----------------------------------------------------------------------------------------------
ORDERING_CALLS = {          # file -> ordering calls (by token, strings and comments left out) it makes through the patched API
    "ops.py": 6, "ffb6d.py": 5, "pyramid.py": 5, "geoMatch.py": 1, "infer.py": 9, "train_graph.py": 3, "train_lm.py": 1,
}
_METHODS = ("record", "wait", "synchronize", "wait_event", "wait_stream", "record_event", "record_stream")


def test_every_ordering_call_of_the_package_goes_through_the_patched_api():
    """audited() sees an ordering call only if it is one of stream_audit.SYNC_API, made from Python.  So: the attribute calls with
    those names are where this table says they are (a new site makes the author look here), and nothing in the package reaches a
    stream or an event another way (the runtime through ctypes, torch._C, an external stream, torch's stream / event wrappers of
    other back ends).  `.wait(` and `.record(` are matched by name alone: a new one on another kind of object shows up here too."""
    found, other = {}, []
    for fn in sorted(os.listdir(sa.PKG)):
        if not fn.endswith(".py"):
            continue
        with open(os.path.join(sa.PKG, fn)) as f:
            text = f.read()
        toks = [t for t in tokenize.generate_tokens(io.StringIO(text).readline) if t.type in (tokenize.NAME, tokenize.OP)]
        n = sum(1 for a, b, c in zip(toks, toks[1:], toks[2:]) if a.string == "." and b.string in _METHODS and c.string == "(")
        if n:
            found[fn] = n
        names = {t.string for t in toks if t.type == tokenize.NAME}
        other += [(fn, w) for w in ("hipStreamWaitEvent", "hipEventRecord", "hipStreamSynchronize", "hipDeviceSynchronize", "ExternalStream",
                                    "_cuda_synchronize", "_CudaEventBase", "_CudaStreamBase", "default_stream", "set_stream",
                                    "hipEventSynchronize") if w in names]
    assert found == ORDERING_CALLS
    assert not other
    assert len(sa.SYNC_API) == 9
    for name in sa.SYNC_API:          # every patched name exists where audited() patches it
        owner = torch
        for part in name.split(".")[1:]:
            owner = getattr(owner, part)
        assert callable(owner), name


# ---- job structures ------------------------------------------------------------------------------------------------------------
def test_struct_const_table_comes_from_the_header():
    assert sa.STRUCT_CONST["gdm_knn_job"] == {"support": True, "query": True, "idx": False, "d2": False}
    assert sa.STRUCT_CONST["gdm_copy_job"] == {"dst": False, "src": True}
    assert sa.STRUCT_CONST["gdm_pw_seg"] == {"x": True, "idx": True}
    assert sa.STRUCT_CONST["gdm_pw_job"] == {"x": True, "wt": True, "out": False}
    assert set(sa.EXTENT) == {(s, f) for s, fields in sa.STRUCT_CONST.items() for f in fields}


def _cpu_audit():
    """The recorder on host tensors: one stream called "main", and a stand-in for the library that does nothing."""
    return sa.audited(device_type="cpu", current_stream=lambda: "main", role=lambda s: s, sync_calls=False, target=lambda name, *args: None)


def test_job_structure_round_trip_on_host_memory():
    """A KnnJob array whose pointers are addresses of registered CPU tensors: every field resolves to its tensor, with the bytes
    the job's sizes give, const from the header; an address outside every tensor is reported, not dropped."""
    from geometric_aware_dense_matching_amd import ops
    B, N, S, Q, K = 2, 40, 24, 10, 4
    cloud = torch.zeros(B, N, 3)
    sup, qry = cloud[:, :S], cloud[:, :Q]                       # prefix slices: the batch stride stays N * 3
    slab = torch.zeros(B * Q * K + 64 + B * Q, dtype=torch.int32)
    arr = (_lib.KnnJob * 2)()
    for k, (off, kk) in enumerate(((0, K), (B * Q * K + 64, 1))):
        a = arr[k]
        a.support, a.query, a.idx, a.d2 = sup.data_ptr(), qry.data_ptr(), slab.data_ptr() + 4 * off, None
        a.support_bstride, a.query_bstride, a.S, a.Q, a.K = sup.stride(0), qry.stride(0), S, Q, kk
    ws = torch.zeros(64, dtype=torch.uint8)
    with _cpu_audit() as tr:
        tr.register([cloud, slab])
        ops.call("gdm_knn_jobs_ws_hip", arr, 2, B, ws, 64)
    assert not tr.unresolved
    (e,) = [e for e in tr.log if e.kind == "access"]
    assert e.name == "gdm_knn_jobs_ws_hip" and e.stream == "main"
    cp, sp = cloud.untyped_storage().data_ptr(), slab.untyped_storage().data_ptr()
    reads = {s.label: s for s in e.reads}
    writes = {s.label: s for s in e.writes}
    assert set(reads) == {"jobs[0].support", "jobs[0].query", "jobs[1].support", "jobs[1].query"}
    assert reads["jobs[0].support"][:3] == (cp, 0, 4 * (N * 3 + S * 3)) and reads["jobs[1].query"][:3] == (cp, 0, 4 * (N * 3 + Q * 3))
    assert set(writes) == {"jobs[0].idx", "jobs[1].idx", "workspace"}
    assert writes["jobs[0].idx"][:3] == (sp, 0, 4 * B * Q * K)
    assert writes["jobs[1].idx"][:3] == (sp, 4 * (B * Q * K + 64), 4 * (B * Q * K + 64 + B * Q))
    assert writes["jobs[0].idx"].hi <= writes["jobs[1].idx"].lo                              # two arrays of one slab do not collide
    # an address in no registered tensor, and one whose extent runs past its tensor's end
    arr[0].idx = slab.data_ptr() + slab.numel() * 4 + (1 << 20)
    arr[1].K = K
    with _cpu_audit() as tr:
        tr.register([cloud, slab])
        ops.call("gdm_knn_jobs_ws_hip", arr, 2, B, ws, 64)
    assert sorted(u[1] for u in tr.unresolved) == ["jobs[0].idx", "jobs[1].idx"]
    assert sa.analyse(tr.log, unresolved=tr.unresolved).unresolved


def test_copy_jobs_pointer_arrays_and_bare_addresses():
    from geometric_aware_dense_matching_amd import ops
    src = torch.zeros(2, 8, 8, 3)
    view = src[:, ::2, ::2, :]
    dst = torch.zeros(view.shape)
    arr = (_lib.CopyJob * 1)(_lib.CopyJob(dst.data_ptr(), view.data_ptr(), view.stride(0), view.stride(1), view.stride(2), *view.shape))
    layers = [torch.zeros(128, 128), torch.zeros(128, 128)]
    w_arr = (ctypes.c_void_p * 2)(*[t.data_ptr() for t in layers])
    none_arr = (ctypes.c_void_p * 2)(None, None)
    act = (ctypes.c_int * 2)(0, 1)
    a, out = torch.zeros(1, 128, 16), torch.zeros(1, 128, 16)
    with _cpu_audit() as tr:
        tr.register([src, dst] + layers)
        ops.call("gdm_copy_jobs_hip", arr, 1)
        ops.call("gdm_point_heads2_hip", a, None, 128, None, None, 0, 1, 16, 2, w_arr, none_arr, none_arr, act, 1, -1, None, None, 0, out, None)
    assert not tr.unresolved
    copy, heads = [e for e in tr.log if e.kind == "access"]
    assert [(s.label, s.lo, s.hi) for s in copy.writes] == [("jobs[0].dst", 0, dst.numel() * 4)]
    assert [(s.label, s.lo, s.hi) for s in copy.reads] == [("jobs[0].src", 0, 4 * (1 * 192 + 3 * 48 + 3 * 6 + 3))]
    assert sorted(s.label for s in heads.reads) == ["a", "w[0]", "w[1]"] and [s.label for s in heads.writes] == ["out_feat"]
    assert all(s.hi == 128 * 128 * 4 for s in heads.reads if s.label.startswith("w["))     # a bare pointer: to the end of its storage


def test_recorder_logs_aten_reads_writes_and_allocation_streams():
    x = torch.ones(4, 8)
    now = ["main"]
    with sa.audited(device_type="cpu", current_stream=lambda: now[0], role=lambda s: s, sync_calls=False, target=lambda *a: None) as tr:
        y = x * 2                       # fresh output on main
        v = y[1:3]                      # a view: no access
        now[0] = "side0"
        v.add_(1)                       # in-place write of rows 1-2, on the side stream
        z = torch.empty(4)              # an allocation without a kernel
        torch.sum(y[3:], dim=1, out=z[:1].view(1))
    acc = [e for e in tr.log if e.kind == "access"]
    assert [(e.name, e.stream) for e in acc] == [("aten::mul", "main"), ("aten::add_", "side0"), ("aten::sum", "side0")]
    yp = y.untyped_storage().data_ptr()
    assert [(s.storage, s.lo, s.hi) for s in acc[0].writes] == [(yp, 0, 128)] and acc[0].reads[0].storage == x.untyped_storage().data_ptr()
    assert [(s.storage, s.lo, s.hi, s.label) for s in acc[1].writes] == [(yp, 32, 96, "self")]
    assert (yp, 96, 128) in [(s.storage, s.lo, s.hi) for s in acc[2].reads] and acc[2].writes[0].label == "out"
    allocs = {e.storage: e.stream for e in tr.log if e.kind == "alloc"}
    assert allocs == {yp: "main", z.untyped_storage().data_ptr(): "side0"}                  # x existed before: no entry
    rep = sa.analyse(tr.log, exceptions={})
    assert [(v.what, v.first[0], v.second[0]) for v in rep.r1] == [("write-then-write", "aten::mul", "aten::add_"),
                                                                   ("write-then-read", "aten::mul", "aten::sum")]
    assert [v.what for v in rep.r2] == ["no record_stream(side0)"]


def test_item_is_a_read_and_a_host_wait_for_its_stream():
    x = torch.ones(4)
    with _cpu_audit() as tr:
        x[2].item()
    assert [(e.kind, getattr(e, "name", None) or e.op) for e in tr.log] == [("access", "aten::_local_scalar_dense"), ("sync", "sync_stream")]
    assert [(s.lo, s.hi) for s in tr.log[0].reads] == [(8, 12)] and tr.log[1].stream == "main"


def test_audited_undoes_every_patch():
    import importlib
    mods = [importlib.import_module("geometric_aware_dense_matching_amd." + m) for m in sa.guard_bands.MODULES]
    before = ([m.call for m in mods], torch.cuda.Event.record, torch.cuda.Stream.wait_stream, torch.cuda.synchronize, torch.Tensor.record_stream,
              "record_stream" in torch.Tensor.__dict__)
    with pytest.raises(ZeroDivisionError):
        with sa.audited(device_type="cpu", current_stream=lambda: "main", role=lambda s: s):
            assert torch.cuda.Event.record is not before[1] and mods[0].call is not before[0][0]
            1 / 0
    after = ([m.call for m in mods], torch.cuda.Event.record, torch.cuda.Stream.wait_stream, torch.cuda.synchronize, torch.Tensor.record_stream,
             "record_stream" in torch.Tensor.__dict__)
    assert before == after
    assert torch.utils._python_dispatch._get_current_dispatch_mode() is None
