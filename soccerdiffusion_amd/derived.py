"""When is a copy derived from the weights still valid?  The one place that knows.

Split fp16 planes, folded BatchNorm vectors, the C-ABI pointer struct, a prepared sampler workspace and a captured graph are all derived
from parameters, and each is valid while its sources are what they were.  Four facts decide that:

* a tensor's version counter (every torch in-place op moves it);
* its address (``p.data = other`` and ``.to(device)`` move it and leave the counter alone; addresses are unique across host and
  devices within a process);
* ``weights_generation()``: FusedAdamW and replayed training graphs rewrite parameters through raw pointers, which moves neither, so
  every such update calls ``bump_weights_generation()``;
* a tensor made under ``torch.inference_mode()`` has no counter: nothing derived from it is ever taken as current.

What the rule cannot see: a write through ``p.data`` in place (``p.data.mul_(...)``, an EMA update) moves neither counter nor address.
``bump_weights_generation()`` is the explicit invalidate for that.

Derived values live here, keyed weakly by the object that owns the sources, never on the modules: ``copy.deepcopy`` and pickling of a
model neither carry nor share them."""

from __future__ import annotations

import weakref

_generation = 0
_store: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()   # owner -> {name: (key, value) | dict}


def weights_generation() -> int:
    return _generation


def bump_weights_generation() -> None:
    global _generation
    _generation += 1


def versions(*tensors):
    """The per-tensor half of ``version_key``, or None when a tensor has no version counter: the whole key of copies whose owner is the
    only one to rewrite their sources through raw pointers and refreshes them itself each time (a FusedAdamW's planes: the generation
    moves with every optimizer's step, another one's included)."""
    try:
        return tuple([t._version for t in tensors])
    except RuntimeError:
        return None


def version_key(*tensors):
    """(generation, versions), or None when a tensor has no version counter.  For long per-call lists whose addresses something else
    already covers; everything else takes ``source_key``."""
    v = versions(*tensors)
    return None if v is None else (_generation, v)


def source_key(*tensors):
    """(generation, (address, version) per tensor), or None when a tensor has no version counter."""
    try:
        return _generation, tuple([(t.data_ptr(), t._version) for t in tensors])
    except RuntimeError:
        return None


def current(stored, key) -> bool:
    """A None key (a source without a counter) is never current."""
    return key is not None and stored == key


def _entries(owner) -> dict:
    per = _store.get(owner)
    if per is None:
        per = _store[owner] = {}
    return per


def derived(owner, name: str, sources, build):
    """The value stored for (owner, name) while ``source_key(*sources)`` is current; otherwise ``build(previous value or None)``, stored
    under the new key.  ``build`` gets the previous value so that planes are repacked in place: captured graphs hold their addresses."""
    per = _entries(owner)
    key = source_key(*sources)
    hit = per.get(name)
    if hit is not None and current(hit[0], key):
        return hit[1]
    value = build(None if hit is None else hit[1])
    per[name] = (key, value)
    return value


def cache(owner, name: str) -> dict:
    """A plain per-owner dict (loop samplers, captured graphs, pointer structs) for entries that carry keys of their own."""
    return _entries(owner).setdefault(name, {})
