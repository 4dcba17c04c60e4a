"""soccerdiffusion_amd/derived.py: the one staleness rule for copies derived from the weights (version counter, address,
ops.weights_generation(), no counter under inference_mode), the weak store that keeps them off the modules, and what that buys:
copy.deepcopy / pickle of a model whose C-ABI descriptors have been built."""

import copy
import gc
import pickle

import pytest
import torch
from torch import nn

from soccerdiffusion_amd import derived as dv


class _Owner:
    pass


def _counting():
    calls = []

    def build(old):
        calls.append(old)
        return len(calls)

    return calls, build


def test_rule_hit_and_the_three_ways_to_miss():
    from soccerdiffusion_amd import ops

    owner, (calls, build) = _Owner(), _counting()
    a, b = torch.zeros(4), torch.ones(3)
    get = lambda: dv.derived(owner, "x", (a, b), build)
    assert get() == 1 and get() == 1 and calls == [None]            # unchanged sources: a hit
    b.add_(1.0)                                                     # a torch in-place op
    assert get() == 2 and get() == 2 and calls == [None, 1]         # ... build receives the previous value
    version, ptr = a._version, a.data_ptr()
    a.data = torch.full((4,), 2.0)                                  # new storage behind the same counter
    assert a._version == version and a.data_ptr() != ptr
    assert get() == 3 and get() == 3
    assert ops.weights_generation() == dv.weights_generation()      # (ops keeps both names)
    ops.bump_weights_generation()
    assert get() == 4 and get() == 4
    assert dv.derived(owner, "y", (a,), build) == 5 and get() == 4  # names do not share entries


def test_source_without_a_version_counter_is_never_current():
    with torch.inference_mode():
        t = torch.ones(3)
    with pytest.raises(RuntimeError):
        t._version
    assert dv.version_key(t) is None and dv.source_key(torch.zeros(1), t) is None
    assert not dv.current(None, None) and not dv.current(dv.version_key(torch.zeros(1)), None)
    owner, (calls, build) = _Owner(), _counting()
    assert [dv.derived(owner, "x", (t,), build) for _ in range(3)] == [1, 2, 3]
    assert calls == [None, 1, 2]


def test_keys():
    a, b = torch.zeros(2), torch.zeros(2)
    g = dv.weights_generation()
    assert dv.version_key(a, b) == (g, (a._version, b._version))
    assert dv.source_key(a, b) == (g, ((a.data_ptr(), a._version), (b.data_ptr(), b._version)))
    assert dv.current(dv.source_key(a), dv.source_key(a)) and not dv.current(dv.source_key(a), dv.source_key(b))


def test_store_is_weak_and_not_copied():
    owner = nn.Linear(2, 2)
    dv.derived(owner, "x", (owner.weight,), lambda old: "planes")
    dv.cache(owner, "loop")["k"] = 1
    assert dv.cache(owner, "loop") == {"k": 1}
    twin = copy.deepcopy(owner)
    assert twin not in dv._store and dv.cache(twin, "loop") == {}
    n = len(dv._store)
    del owner
    gc.collect()
    assert len(dv._store) == n - 1


def _pack_all(model: nn.Module) -> int:
    return sum(1 for mod in model.modules() if hasattr(mod, "packed") and mod.packed() is not None)


def _models():
    from soccerdiffusion_amd import cli
    from soccerdiffusion_amd.ml.model.decoder import DiffusionActionGenerator
    from soccerdiffusion_amd.ml.model.encoder.base import BaseEncoder
    from test_gpu_frames_area import DEFAULT_YAML

    return {"decoder": lambda: DiffusionActionGenerator(20, 64, 1, 4, 10), "encoder": lambda: BaseEncoder(20, 5, 64, 1, 4, 20),
            "default.yaml": lambda: cli.build_model(DEFAULT_YAML)}


@pytest.mark.parametrize("which", ["decoder", "encoder", "default.yaml"])
def test_deepcopy_and_pickle_after_packed(which):
    """The descriptor holds ctypes pointers; kept on the module (as it was) both calls raise ``ValueError: ctypes objects containing
    pointers cannot be pickled``."""
    model = _models()[which]()
    assert _pack_all(model) == {"decoder": 1, "encoder": 1, "default.yaml": 5}[which]
    assert not any(hasattr(mod, "_packed") or hasattr(mod, "_packed_sig") for mod in model.modules())
    twin = copy.deepcopy(model)
    again = pickle.loads(pickle.dumps(model))
    for other in (twin, again):
        pairs = [(a, b) for a, b in zip(model.modules(), other.modules()) if hasattr(a, "packed")]
        assert pairs
        for a, b in pairs:
            assert b.packed() is not a.packed() and b.packed() is b.packed()
            assert b.packed().struct.emb_w == b.embedding.weight.data_ptr() != a.embedding.weight.data_ptr()
        assert all(torch.equal(p, q) for p, q in zip(model.state_dict().values(), other.state_dict().values()))
