"""The one cache for tensors derived from parameters (folded BatchNorms, transposed / packed / split weights, ...).

Every derived value lives in `owner.__dict__["_gdm_derived"][slot]`: outside `_parameters` / `_buffers`, so it never reaches
`state_dict()`, and inside `__dict__`, so `copy.deepcopy` carries it along with the copy's own tensors as its dependencies.

Not seen: a write through `.data` (`w.data.mul_(2)`) leaves `_version` and `data_ptr()` as they were.  Call `invalidate(model)`
after one.  In-place operations under `torch.no_grad()`, `load_state_dict`, optimizer steps and `.to()` / `.double()` are seen."""
import torch

_STORE = "_gdm_derived"


def derived(owner, slot, deps, make, extra=()):
    """make() cached on `owner` under `slot` until a tensor in `deps` is replaced, modified in place or moved.

    A hit needs the same dep OBJECTS (`is`), equal `(_version, data_ptr())` of each, and `extra == ` the stored one.  So pass the
    parameter, the buffer or the cached parent value itself -- never a fresh view such as `w.reshape(64, 64)`, which misses on
    every call.  make() runs under `torch.no_grad()`; whatever it returns is cached, `None` included.  `owner` is a module, or the
    weight tensor itself (then the owner, as its own dep, is not referenced from its own store)."""
    store = owner.__dict__.get(_STORE)
    if store is None:
        store = owner.__dict__[_STORE] = {}
    key = tuple((t._version, t.data_ptr()) for t in deps)
    entry = store.get(slot)
    if (entry is None or entry[1] != key or entry[2] != extra
            or any(held is not (None if t is owner else t) for held, t in zip(entry[0], deps))):
        with torch.no_grad():
            value = make()
        entry = store[slot] = (tuple(None if t is owner else t for t in deps), key, extra, value)
    return entry[3]


def invalidate(module):
    """Drop every derived value held by `module`, its submodules and their parameters (after a write through .data)."""
    for m in module.modules():
        m.__dict__.pop(_STORE, None)
    for p in module.parameters():
        p.__dict__.pop(_STORE, None)
