"""A happens-before audit of the step's stream ordering: who touched which bytes on which stream, and which waits were issued.

The forked step spreads its kernels over up to five streams, and nothing orders those but a protocol written by hand in Python
(ops.fork, ffb6d._Lanes.exchange, pyramid.wait_ready, the KEEP lists, record_stream calls, scratch pools keyed by stream role).  A
mistake there is an unordered read / write pair, and a comparison of results sees it only when the timing of that run exposes it.
Whether two accesses are ordered is a property of the HOST program's calls, so it is decided here from a log of them, exactly and
without timing.  Nothing runs on the device on behalf of the audit: it never synchronises and never allocates there.

  audited()       a context that records, and undoes every patch on exit:
                    * the ordering calls, patched on the classes (torch.cuda.Event.record / wait / synchronize, torch.cuda.Stream.
                      wait_event / wait_stream / record_event / synchronize, torch.cuda.synchronize, torch.Tensor.record_stream);
                    * every aten op, through a TorchDispatchMode: the current stream, the tensors read, the tensors written (the
                      schema's alias_info.is_write plus the fresh outputs).  A storage that first appears as a fresh output was
                      allocated on that stream during the audit; one that first appears as an input existed before it;
                    * every `*_hip` library call, by replacing `call` in the modules that bind it (guard_bands.MODULES): a pointer
                      that include/gdm.h declares `const` is a read, any other a write.  Pointers inside job structures
                      (gdm_knn_job, gdm_copy_job, gdm_pw_seg, gdm_pw_job), in the layer arrays of gdm_point_heads2_hip and bare
                      addresses are resolved to the registered storage that contains them; one that resolves to nothing is kept in
                      `unresolved` and fails the audit: it is unknown memory, not "no access".
                  An access is a byte interval of a storage (storage_offset to the furthest reachable element), so that disjoint
                  views of one allocation do not collide, and carries the op or entry name and the nearest package frames.
                  While it records, the context holds a reference to every storage it has seen: no block is freed and handed out
                  again under the audit, so a storage's address names it.
  analyse(log)    a pure function of the log (re-run it on an edited log):
                    R1 ordering   two accesses with overlapping bytes on different streams, at least one a write, must be ordered
                                  by happens-before in program direction (read-after-write, write-after-read, write-after-write);
                    R2 lifetime   ops.fork's rule: a storage allocated during the audit and accessed on a stream other than its
                                  allocation stream must have record_stream(that stream) logged.  Storages that existed before
                                  (parameters, static inputs, pool buffers) are exempt: R1 is all that protects them.
                  One vector clock per stream: an access on s is stamped (s, ++c_s); Event.record(s) snapshots VC[s]; a wait joins
                  the snapshot of the event's LATEST record into VC[waiter]; wait_stream is record + wait; the synchronize calls
                  join into a host clock that every later access sees.  (s1, c1) happens before an access on s2 iff s1 == s2 or
                  VC[s2][s1] >= c1 when that access is issued.  No implicit ordering through the default stream is assumed.

What the audit cannot see: an access a kernel makes outside the arguments it was given (tests/guard_bands.py looks for those); the
exact bytes behind a bare pointer (taken to the end of its storage, an over-approximation); anything the hardware does.
torch's own stream-race tracer is not used: its process-wide trace hooks cannot be removed again."""
import bisect
import collections
import contextlib
import ctypes
import linecache
import os
import re
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode

import guard_bands
from geometric_aware_dense_matching_amd import _lib

PKG = os.path.dirname(os.path.abspath(_lib.__file__))

# ---- the log -------------------------------------------------------------------------------------------------------------------
Span = collections.namedtuple("Span", "storage lo hi label")                      # bytes [lo, hi) of a storage; label: parameter / role
Access = collections.namedtuple("Access", "kind stream name site reads writes")   # kind "access"; reads / writes: tuples of Span
Sync = collections.namedtuple("Sync", "kind op stream event site call")           # kind "sync"; op: record wait sync_stream sync_event sync_all
Keep = collections.namedtuple("Keep", "kind storage stream site")                 # kind "keep": record_stream(stream) of a storage
Alloc = collections.namedtuple("Alloc", "kind storage stream name site")          # kind "alloc": first seen as a fresh output


def access(stream, name, reads=(), writes=(), site=()):
    return Access("access", stream, name, tuple(site), tuple(Span(*s) for s in reads), tuple(Span(*s) for s in writes))


def record(stream, event, site=(), call="record"):
    return Sync("sync", "record", stream, event, tuple(site), call)


def wait(stream, event, site=(), call="wait"):
    return Sync("sync", "wait", stream, event, tuple(site), call)


def wait_stream(waiter, other, site=(), _n=[0]):
    """Stream.wait_stream(other): an event of its own, recorded on `other` and waited for by `waiter`."""
    _n[0] += 1
    ev = ("wait_stream", _n[0])
    return [record(other, ev, site, "wait_stream"), wait(waiter, ev, site, "wait_stream")]


def synchronize(stream=None, event=None, site=()):
    op = "sync_stream" if stream is not None else "sync_event" if event is not None else "sync_all"
    return Sync("sync", op, stream, event, tuple(site), "synchronize")


def keep(storage, stream, site=()):
    return Keep("keep", storage, stream, tuple(site))


def alloc(storage, stream, name="alloc", site=()):
    return Alloc("alloc", storage, stream, name, tuple(site))


# ---- exceptions: (entry or op, parameter or tensor role) -> the written reason.  A pooled scratch buffer or a tensor named in a
# use / join / exchange list may not be excepted.
EXCEPTIONS = {}


class Violation(collections.namedtuple("Violation", "rule first second what count")):
    """first / second: (entry or op, stream role, package frames, parameter or tensor role) of the two accesses (R2: the allocation
    and the first access on the other stream)."""

    def __str__(self):
        def one(a):
            return "%s `%s` on %s at %s" % (a[0], a[3], a[1], " < ".join(a[2]) or "<outside the package>")
        return "%s %s: %s  ||  %s  (x%d)" % (self.rule, self.what, one(self.first), one(self.second), self.count)


class Report:
    def __init__(self):
        self.r1, self.r2, self.excepted, self.unresolved = [], [], [], []
        self.streams = set()                 # every stream that carries an access
        self.calls = collections.Counter()   # stream -> library calls on it
        self.ordered = set()                 # (writer stream, reader stream) of the cross-stream write-then-read pairs an event orders
        self.accesses = 0
        self.used_exceptions = set()

    @property
    def violations(self):
        return self.r1 + self.r2

    def __str__(self):
        return "\n".join(str(v) for v in self.violations) or "no violation"


def _side(e, sp):
    return (e.name, e.stream, e.site, sp.label)


def analyse(log, exceptions=None, unresolved=()):
    """R1 and R2 over `log` (a list of Access / Sync / Keep / Alloc).  Violations are grouped by the two places they name."""
    exceptions = EXCEPTIONS if exceptions is None else exceptions
    rep = Report()
    rep.unresolved = list(unresolved)
    vc = collections.defaultdict(dict)            # stream -> {stream: clock}
    clock = collections.Counter()
    host = {}                                     # what the host has waited for: every later access sees it
    snaps = {}                                    # event -> the snapshot of its latest record
    past = collections.defaultdict(list)          # storage -> [(stream, clock, lo, hi, is write, entry, span)]
    allocs, kept, first_on = {}, collections.defaultdict(set), collections.defaultdict(dict)
    found = {}

    def join(into, other):
        for k, v in other.items():
            if into.get(k, 0) < v:
                into[k] = v

    def report(rule, what, a, b):
        key = (rule, what, a, b)
        found[key] = found.get(key, 0) + 1

    for e in log:
        if e.kind == "access":
            s = e.stream
            clock[s] += 1
            c = clock[s]
            rep.streams.add(s)
            rep.accesses += 1
            if e.name.startswith("gdm_"):
                rep.calls[s] += 1
            seen = vc[s]
            join(seen, host)
            for is_write, spans in ((False, e.reads), (True, e.writes)):
                for sp in spans:
                    first_on[sp.storage].setdefault(s, (e, sp))
                    for s1, c1, lo, hi, w1, e1, sp1 in past[sp.storage]:
                        if s1 == s or not (w1 or is_write) or hi <= sp.lo or sp.hi <= lo:
                            continue
                        if seen.get(s1, 0) >= c1:
                            if w1 and not is_write:
                                rep.ordered.add((s1, s))
                            continue
                        report("R1", ("write" if w1 else "read") + "-then-" + ("write" if is_write else "read"), _side(e1, sp1), _side(e, sp))
            for is_write, spans in ((False, e.reads), (True, e.writes)):
                for sp in spans:
                    past[sp.storage].append((s, c, sp.lo, sp.hi, is_write, e, sp))
        elif e.kind == "sync":
            if e.op == "record":
                join(vc[e.stream], host)
                snap = dict(vc[e.stream])
                snap[e.stream] = clock[e.stream]
                snaps[e.event] = snap
            elif e.op == "wait":
                join(vc[e.stream], snaps.get(e.event, {}))          # an event never recorded orders nothing
            elif e.op == "sync_stream":
                join(host, vc[e.stream])
                host[e.stream] = max(host.get(e.stream, 0), clock[e.stream])
            elif e.op == "sync_event":
                join(host, snaps.get(e.event, {}))
            elif e.op == "sync_all":
                for t in list(vc) + list(clock):
                    join(host, vc[t])
                    host[t] = max(host.get(t, 0), clock[t])
            else:
                raise ValueError("unknown sync op %r" % (e.op,))
        elif e.kind == "keep":
            kept[e.storage].add(e.stream)
        elif e.kind == "alloc":
            allocs.setdefault(e.storage, e)
        else:
            raise ValueError("unknown log entry %r" % (e,))
    for storage, a in allocs.items():
        for s, (e, sp) in first_on[storage].items():
            if s != a.stream and s not in kept[storage]:
                report("R2", "no record_stream(%s)" % (s,), (a.name, a.stream, a.site, "allocation"), _side(e, sp))
    for (rule, what, a, b), n in found.items():
        v = Violation(rule, a, b, what, n)
        why = [k for k in ((a[0], a[3]), (b[0], b[3])) if k in exceptions]
        if why:
            rep.excepted.append(v)
            rep.used_exceptions.update(why)
        else:
            (rep.r1 if rule == "R1" else rep.r2).append(v)
    return rep


def sites(log, what):
    """The distinct call sites of the waits (what = "wait") or of the record_stream calls (what = "keep") of a log, in order."""
    out = []
    for e in log:
        if (e.kind == "sync" and e.op == "wait" and what == "wait") or (e.kind == "keep" and what == "keep"):
            if e.site not in out:
                out.append(e.site)
    return out


def without(log, what, site):
    """The log with every wait (or every record_stream) issued from `site` removed."""
    return [e for e in log if not (((e.kind == "sync" and e.op == "wait" and what == "wait") or (e.kind == "keep" and what == "keep"))
                                   and e.site == site)]


def sequence(log):
    """(entry / op / sync op, stream role) of every access and ordering call, with every stream that is no side stream named
    "main": what a captured step and the eager step must have in common for the eager audit to speak for the graph."""
    def role(s):
        return s if str(s).startswith("side") else "main"
    out = []
    for e in log:
        if e.kind == "access":
            out.append((e.name, role(e.stream)))
        elif e.kind == "sync":
            out.append((e.call + ":" + e.op, role(e.stream) if e.stream is not None else None))
        elif e.kind == "keep":
            out.append(("record_stream", role(e.stream)))
    return out


# ---- include/gdm.h: which pointer fields of the job structures are const --------------------------------------------------------
def _parse_structs(text):
    """{C struct name: {pointer field: declared const?}} of every `typedef struct` of the header."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    table = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        fields = {}
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            ctype, first, rest = re.fullmatch(r"(.*?)(\w+)((?:\s*,\s*\w+)*)", decl, flags=re.S).groups()
            if "*" in ctype:
                for f in [first] + re.findall(r"\w+", rest):
                    fields[f] = re.search(r"\bconst\b", ctype) is not None
        table[name] = fields
    return table


with open(_lib.HEADER) as _f:
    STRUCT_CONST = _parse_structs(_f.read())
_STRUCT_NAME = {cls: name for name, cls in _lib._STRUCTS.items()}

# bytes reachable through a pointer field: (struct, field) -> f(job, scalars of the call)
EXTENT = {
    ("gdm_knn_job", "support"): lambda j, a: 4 * ((a["B"] - 1) * j.support_bstride + j.S * 3),
    ("gdm_knn_job", "query"): lambda j, a: 4 * ((a["B"] - 1) * j.query_bstride + j.Q * 3),
    ("gdm_knn_job", "idx"): lambda j, a: 4 * a["B"] * j.Q * j.K,
    ("gdm_knn_job", "d2"): lambda j, a: 4 * a["B"] * j.Q * j.K,
    ("gdm_copy_job", "dst"): lambda j, a: 4 * j.B * j.R1 * j.R2 * j.E,
    ("gdm_copy_job", "src"): lambda j, a: 4 * ((j.B - 1) * j.sb + (j.R1 - 1) * j.s1 + (j.R2 - 1) * j.s2 + j.E),
    ("gdm_pw_seg", "x"): lambda j, a: 4 * a["B"] * j.C * j.n_src,
    ("gdm_pw_seg", "idx"): lambda j, a: 4 * a["B"] * a["n"],
    ("gdm_pw_job", "x"): lambda j, a: 4 * a["B"] * a["K"] * j.n,
    ("gdm_pw_job", "wt"): lambda j, a: 4 * a["K"] * a["Cout"],
    ("gdm_pw_job", "out"): lambda j, a: 4 * a["B"] * a["Cout"] * j.n,
}


def job_pointers(name, args):
    """Every address a library call is given outside its tensor arguments: [(label, address, bytes or None, const?)].  Job
    structures are decoded field by field, arrays of pointers element by element; a bare int in a pointer parameter is an address.
    bytes None: the extent is not known (the caller takes it to the end of the storage)."""
    params = _lib.PARAMS[name]
    const = guard_bands.CONST.get(name, {})
    scalars = {p: a for p, a in zip(params, args) if type(a) is int}
    out = []
    for p, a in zip(params, args):
        if isinstance(a, ctypes.Array) and issubclass(a._type_, ctypes.Structure):
            sname = _STRUCT_NAME[a._type_]
            for k, job in enumerate(a):
                for f, ftype in job._fields_:
                    if ftype is ctypes.c_void_p and getattr(job, f):
                        ext = EXTENT.get((sname, f))
                        out.append(("%s[%d].%s" % (p, k, f), getattr(job, f), ext(job, scalars) if ext else None, STRUCT_CONST[sname][f]))
        elif isinstance(a, ctypes.Array) and a._type_ is ctypes.c_void_p:
            out += [("%s[%d]" % (p, k), v, None, const.get(p, False)) for k, v in enumerate(a) if v]
        elif type(a) is int and p in const and a:
            out.append((p, a, None, const[p]))
    return out


# ---- recording -----------------------------------------------------------------------------------------------------------------
_ALLOC_ONLY = re.compile(r"aten::(empty|empty_like|empty_strided|new_empty|new_empty_strided)$")          # a block, and no kernel
_NO_KERNEL = re.compile(r"aten::(record_stream|detach|alias|lift_fresh|is_pinned|sym_\w+|size|stride|storage_offset)$")


def _span_elems(t):
    return 1 + sum((s - 1) * st for s, st in zip(t.shape, t.stride()))


def _tensors(x):
    if isinstance(x, torch.Tensor):
        yield x
    elif isinstance(x, (list, tuple)):
        for y in x:
            yield from _tensors(y)


def _frames(depth=3):
    """The nearest `depth` frames inside the package, as "file.py:function: source line" (no line numbers: they would tie a table
    of sites to every edit above it)."""
    out = []
    f = sys._getframe(1)
    while f is not None and len(out) < depth:
        fn = f.f_code.co_filename
        if fn.startswith(PKG):
            out.append("%s:%s: %s" % (os.path.basename(fn), f.f_code.co_name, linecache.getline(fn, f.f_lineno).strip()))
        f = f.f_back
    return tuple(out)


class Tracker:
    """The log and the registry of storages behind one audited() context."""

    def __init__(self, device_type="cuda", current_stream=None, role=None):
        self.log, self.unresolved = [], []
        self.device_type = device_type
        self._current = current_stream or (lambda: torch.cuda.current_stream())
        self._role_of = role or self._default_role
        self._storages = {}            # address -> (bytes, the storage: held, so the address stays its name)
        self._sorted = None
        self._events = {}              # id(event) -> (number, the event: held, so the id stays its name)
        self._mains = []
        self._depth = 0
        self._n_ws = 0

    # -- names
    def _default_role(self, stream):
        from geometric_aware_dense_matching_amd import ops
        h = stream.cuda_stream
        for (_d, which), st in ops._side_streams.items():
            if st.cuda_stream == h:
                return "side%d" % which
        if h not in self._mains:
            self._mains.append(h)
        k = self._mains.index(h)
        return "main" if k == 0 else "main%d" % (k + 1)

    def stream(self, s=None):
        return self._role_of(self._current() if s is None else s)

    def event(self, ev):
        got = self._events.get(id(ev))
        if got is None:
            got = self._events[id(ev)] = (len(self._events), ev)
        return "event%d" % got[0]

    # -- storages
    def tracked(self, t):
        return isinstance(t, torch.Tensor) and t.device.type == self.device_type and t.numel() > 0 and not t.is_sparse

    def register(self, tensors):
        """Tensors that exist before the audited step (parameters, derived weights, pool buffers, inputs): addresses inside them
        resolve, and they are exempt from R2."""
        for t in tensors:
            if self.tracked(t):
                self._storage(t)

    def _storage(self, t):
        """(address of the tensor's storage, seen before?)"""
        st = t.untyped_storage()
        ptr = st.data_ptr()
        known = ptr in self._storages
        if not known:
            self._storages[ptr] = (st.nbytes(), st)
            self._sorted = None
        return ptr, known

    def span(self, t, label):
        ptr, _ = self._storage(t)
        lo = t.storage_offset() * t.element_size()
        return Span(ptr, lo, lo + _span_elems(t) * t.element_size(), label)

    def resolve(self, address, nbytes, label):
        """The span of `nbytes` (None: to the end of the storage) at a raw address, or None when no registered storage holds it."""
        if self._sorted is None:
            self._sorted = sorted(self._storages)
        k = bisect.bisect_right(self._sorted, address) - 1
        if k < 0:
            return None
        ptr = self._sorted[k]
        size = self._storages[ptr][0]
        lo = address - ptr
        if lo >= size or (nbytes is not None and lo + nbytes > size):
            return None
        return Span(ptr, lo, size if nbytes is None else lo + nbytes, label)

    # -- what the patches call
    def on_op(self, func, args, kwargs, out):
        schema = func._schema
        name = schema.name
        if _NO_KERNEL.match(name):
            return
        if _ALLOC_ONLY.match(name):
            for t in _tensors(out):          # the storage belongs to this stream from here on
                if self.tracked(t) and not self._storage(t)[1]:
                    self.log.append(Alloc("alloc", t.untyped_storage().data_ptr(), self.stream(), name, _frames()))
            return
        reads, writes, inputs = [], [], set()
        sargs = schema.arguments
        given = [(sargs[i], a) for i, a in enumerate(args) if i < len(sargs)]
        given += [(sa, kwargs[sa.name]) for sa in sargs if sa.name in kwargs]
        for sa, a in given:
            w = sa.alias_info is not None and sa.alias_info.is_write
            for t in _tensors(a):
                if self.tracked(t):
                    sp = self.span(t, sa.name)
                    inputs.add(sp.storage)
                    (writes if w else reads).append(sp)
        stream = None
        fresh = aliased = 0
        for k, t in enumerate(_tensors(out)):
            if not self.tracked(t):
                continue
            ptr = t.untyped_storage().data_ptr()
            if ptr in inputs:
                aliased += 1          # a view of an input, or the in-place result (already a write above)
                continue
            fresh += 1
            _, known = self._storage(t)
            stream = stream or self.stream()
            if not known:
                self.log.append(Alloc("alloc", ptr, stream, name, _frames()))
            writes.append(self.span(t, "out%d" % k))
        if not writes and (aliased and not fresh):
            return          # a pure view: metadata only, no kernel
        if reads or writes:
            self.log.append(Access("access", stream or self.stream(), name, _frames(), tuple(reads), tuple(writes)))
            if name == "aten::_local_scalar_dense":          # .item(): the host has waited for that stream
                self.log.append(Sync("sync", "sync_stream", stream or self.stream(), None, _frames(), "Tensor.item"))

    def on_call(self, name, args):
        params = _lib.PARAMS[name]
        const = guard_bands.CONST.get(name, {})
        reads, writes = [], []
        for p, a in zip(params, args):
            if self.tracked(a):
                (reads if const.get(p, False) else writes).append(self.span(a, p))
        site = _frames()
        for label, address, nbytes, is_const in job_pointers(name, args):
            sp = self.resolve(address, nbytes, label)
            if sp is None:
                self.unresolved.append((name, label, address, nbytes, site))
            else:
                (reads if is_const else writes).append(sp)
        self.log.append(Access("access", self.stream(), name, site, tuple(reads), tuple(writes)))

    def on_sync(self, entries):
        self.log += entries


class _Mode(TorchDispatchMode):
    def __init__(self, tracker):
        super().__init__()
        self.tracker = tracker

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        out = func(*args, **kwargs)
        self.tracker.on_op(func, args, kwargs, out)
        return out


def _patches(tr):
    """[(owner, attribute, replacement)]: the ordering calls, on the classes.  torch's own Stream methods call each other (wait_stream
    is wait_event(record_event()), wait_event is event.wait): only the outermost call is logged, as the primitives it stands for."""
    E, S = torch.cuda.Event, torch.cuda.Stream

    def outer(orig, entries):
        def patched(*a, **kw):
            if tr._depth:
                return orig(*a, **kw)
            tr._depth += 1
            try:
                ret = orig(*a, **kw)
            finally:
                tr._depth -= 1
            tr.on_sync(entries(ret, _frames(), *a, **kw))
            return ret
        return patched

    def ev_record(ret, site, self, stream=None):
        return [record(tr.stream(stream), tr.event(self), site, "Event.record")]

    def ev_wait(ret, site, self, stream=None):
        return [wait(tr.stream(stream), tr.event(self), site, "Event.wait")]

    def ev_sync(ret, site, self):
        return [Sync("sync", "sync_event", None, tr.event(self), site, "Event.synchronize")]

    def st_wait_event(ret, site, self, event):
        return [wait(tr.stream(self), tr.event(event), site, "Stream.wait_event")]

    def st_wait_stream(ret, site, self, stream):
        tr._n_ws += 1
        ev = "wait_stream%d" % tr._n_ws
        return [record(tr.stream(stream), ev, site, "Stream.wait_stream"), wait(tr.stream(self), ev, site, "Stream.wait_stream")]

    def st_record_event(ret, site, self, event=None):
        return [record(tr.stream(self), tr.event(ret), site, "Stream.record_event")]

    def st_sync(ret, site, self):
        return [Sync("sync", "sync_stream", tr.stream(self), None, site, "Stream.synchronize")]

    def dev_sync(ret, site, device=None):
        return [Sync("sync", "sync_all", None, None, site, "torch.cuda.synchronize")]

    def rec_stream(ret, site, self, stream):
        if not tr.tracked(self):
            return []
        return [Keep("keep", tr._storage(self)[0], tr.stream(stream), site)]

    return [(E, "record", outer(E.record, ev_record)), (E, "wait", outer(E.wait, ev_wait)), (E, "synchronize", outer(E.synchronize, ev_sync)),
            (S, "wait_event", outer(S.wait_event, st_wait_event)), (S, "wait_stream", outer(S.wait_stream, st_wait_stream)),
            (S, "record_event", outer(S.record_event, st_record_event)), (S, "synchronize", outer(S.synchronize, st_sync)),
            (torch.cuda, "synchronize", outer(torch.cuda.synchronize, dev_sync)),
            (torch.Tensor, "record_stream", outer(torch.Tensor.record_stream, rec_stream))]


_ABSENT = object()
SYNC_API = ("torch.cuda.Event.record", "torch.cuda.Event.wait", "torch.cuda.Event.synchronize", "torch.cuda.Stream.wait_event",
            "torch.cuda.Stream.wait_stream", "torch.cuda.Stream.record_event", "torch.cuda.Stream.synchronize", "torch.cuda.synchronize",
            "torch.Tensor.record_stream")


@contextlib.contextmanager
def audited(known=(), device_type="cuda", current_stream=None, role=None, target=None, sync_calls=True):
    """Record everything inside the context into the Tracker it yields; every patch is undone on exit.  known: the tensors that
    exist already (Tracker.register).  device_type / current_stream / role / target / sync_calls let the CPU tests drive the
    recorder on host tensors with a stand-in for the library."""
    import importlib
    tr = Tracker(device_type, current_stream, role)
    tr.register(known)
    real = target or _lib.call

    def call(name, *args):
        if name.endswith("_hip"):
            tr.on_call(name, args)
        return real(name, *args)

    saved = []
    mods = [importlib.import_module("geometric_aware_dense_matching_amd." + m) for m in guard_bands.MODULES]
    try:
        for m in mods:
            saved.append((m, "call", m.__dict__["call"]))
            setattr(m, "call", call)
        for owner, attr, new in (_patches(tr) if sync_calls else ()):
            saved.append((owner, attr, owner.__dict__.get(attr, _ABSENT)))          # (record_stream is inherited from the C base class)
            setattr(owner, attr, new)
        with _Mode(tr):
            yield tr
    finally:
        for owner, attr, old in reversed(saved):
            if old is _ABSENT:
                delattr(owner, attr)
            else:
                setattr(owner, attr, old)
        tr._storages, tr._events = {}, {}          # the log stays; the storages and events it held go


def collect_tensors(*roots, depth=64):
    """Every tensor reachable from `roots` through modules, dicts, lists, tuples, objects with __dict__ or __slots__ and the
    __dict__ of tensors themselves (derived values cached on a weight): what exists before an audited step."""
    out, seen = [], set()

    def walk(x, d):
        if id(x) in seen or d > depth or x is None or isinstance(x, (str, bytes, int, float, bool, type)):
            return
        seen.add(id(x))
        if isinstance(x, torch.Tensor):
            out.append(x)
            walk(getattr(x, "__dict__", None), d + 1)
        elif isinstance(x, dict):
            for v in x.values():
                walk(v, d + 1)
        elif isinstance(x, (list, tuple, set, frozenset)):
            for v in x:
                walk(v, d + 1)
        elif isinstance(x, (torch.cuda.Stream, torch.cuda.Event)) or callable(x) and not isinstance(x, torch.nn.Module):
            return
        else:
            walk(getattr(x, "__dict__", None), d + 1)
            for name in getattr(type(x), "__slots__", ()):
                walk(getattr(x, name, None), d + 1)
    for r in roots:
        walk(r, 0)
    return out
