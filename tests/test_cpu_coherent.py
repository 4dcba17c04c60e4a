"""The draw that continues the previous plan (sd_select_coherent, ops.select_coherent, PolicySession(select="coherent"), cli rollout
--select): everything that needs no GPU - the symbol and the header, the argument errors raised before any launch, the fp64 reference
against a brute-force loop, the weight and lam arithmetic of the Python layer, the command line and plan_change_rms."""

import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import coherent_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "soccerdiffusion_hip.h")


def test_symbol_resolves_and_the_abi_version_stays():
    from soccerdiffusion_amd import _lib

    lib = _lib.load()
    fn = lib.sd_select_coherent
    assert fn.restype is C.c_int and len(fn.argtypes) == 14
    assert fn.argtypes[12] is C.c_float
    assert lib.sd_abi_version() == 1   # additive: the version stays


def test_header_carries_the_prototype():
    text = open(HEADER).read()
    flat = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert ("int sd_select_coherent(const float *x, const float *prev, const int32_t *robots , const float *w, int32_t *index, "
            "float *out , float *cost , int C, int G, int T, int J, int shift, float lam, void *stream);") in flat
    assert re.search(r"#define\s+SD_ABI_VERSION\s+1\b", text)
    assert "sd_select_medoid(const float *x, int32_t *index, float *out" in text   # the medoid's prototype is untouched


def _buf(n=4):
    return C.cast((C.c_float * n)(), C.c_void_p)


def test_argument_errors_return_badarg_without_a_device():
    from soccerdiffusion_amd import _lib

    lib = _lib.load()
    x, prev, w, index, other = (_buf() for _ in range(5))
    ok = dict(x=x, prev=prev, robots=None, w=w, index=index, out=None, cost=None, C=2, G=2, T=10, J=20, shift=5, lam=0.0)

    def call(**kw):
        a = {**ok, **kw}
        return lib.sd_select_coherent(a["x"], a["prev"], a["robots"], a["w"], a["index"], a["out"], a["cost"], a["C"], a["G"], a["T"], a["J"],
                                      a["shift"], a["lam"], None)

    for name in ("x", "prev", "w", "index"):
        assert call(**{name: None}) == -1, name
        assert b"sd_select_coherent" in lib.sd_last_error()
    for kw in (dict(C=0), dict(G=0), dict(G=65), dict(T=0), dict(J=0), dict(shift=-1), dict(shift=10), dict(shift=11)):
        assert call(**kw) == -1, kw
    for lam in (-1.0, -1e-30, float("nan"), float("inf")):
        assert call(lam=lam) == -1, lam
        assert b"lam" in lib.sd_last_error()
    for kw in (dict(out=x), dict(out=prev), dict(cost=x), dict(cost=prev)):
        assert call(**kw) == -1, kw
        assert b"alias" in lib.sd_last_error()
    # an overlap that is not an equal pointer: out one float into x's extent
    inside = C.c_void_p(x.value + 4)
    assert call(out=inside) == -1 and call(cost=inside) == -1


def test_ops_value_errors_come_before_any_launch():
    """CPU tensors throughout: a call that got as far as the device check would raise RuntimeError, not ValueError."""
    from soccerdiffusion_amd import ops

    x, prev = torch.zeros(6, 10, 20), torch.zeros(3, 10, 20)
    for bad in (0, 65, True, 2.0):
        with pytest.raises(ValueError, match="draws"):
            ops.select_coherent(x, bad, prev, 5)
    with pytest.raises(ValueError, match="draws per context|expected"):
        ops.select_coherent(torch.zeros(7, 10, 20), 2, prev, 5)
    with pytest.raises(ValueError, match="prev"):
        ops.select_coherent(x, 2, torch.zeros(3, 10, 19), 5)
    with pytest.raises(ValueError, match="prev"):
        ops.select_coherent(x, 2, torch.zeros(4, 10, 20), 5)      # four plans for three contexts and no robots=
    for bad in (-1, 10, 2.0, True):
        with pytest.raises(ValueError, match="shift"):
            ops.select_coherent(x, 2, prev, bad)
    for bad in (0.0, -0.5, 1.5, float("nan"), "x"):
        with pytest.raises(ValueError, match="decay"):
            ops.select_coherent(x, 2, prev, 5, decay=bad)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="contrast"):
            ops.select_coherent(x, 2, prev, 5, contrast=bad)
    with pytest.raises(ValueError, match="row_weights"):
        ops.select_coherent(x, 2, prev, 5, row_weights=torch.ones(9))
    with pytest.raises(ValueError, match="row_weights"):
        ops.select_coherent(x, 2, prev, 5, row_weights=-torch.ones(10))
    with pytest.raises(ValueError, match="robots"):
        ops.select_coherent(x, 2, torch.zeros(4, 10, 20), 5, robots=[0, 1, 4])
    with pytest.raises(ValueError, match="robots"):
        ops.select_coherent(x, 2, torch.zeros(4, 10, 20), 5, robots=[0, 1, 1])


def test_check_select():
    from soccerdiffusion_amd.session import SELECTORS, PolicySession

    assert SELECTORS == ("medoid", "coherent")
    assert PolicySession.check_draws(8, "coherent", False) == (8, "coherent")
    assert PolicySession.check_select("medoid", 10, 10, 4, 0.5, 0.0) == (0.5, 0.0)      # the medoid needs no overlap
    assert PolicySession.check_select("coherent", 10, 5, 4, 1, 2) == (1.0, 2.0)
    assert PolicySession.check_select("coherent", 10, 9, 1, 0.25, 0.0) == (0.25, 0.0)
    with pytest.raises(ValueError, match="overlap"):
        PolicySession.check_select("coherent", 10, 10, 4, 0.5, 0.0)
    with pytest.raises(ValueError, match="select"):
        PolicySession.check_select("mean", 10, 5, 4, 0.5, 0.0)
    for bad in (0.0, -0.1, 1.0001, float("nan")):
        with pytest.raises(ValueError, match="decay"):
            PolicySession.check_select("coherent", 10, 5, 4, bad, 0.0)
    for bad in (-1e-9, float("nan")):
        with pytest.raises(ValueError, match="contrast"):
            PolicySession.check_select("coherent", 10, 5, 4, 0.5, bad)

    class Model:   # the constructor validates before it looks at a device: no parameters are touched
        trajectory_prediction_length = 10
        num_joints = 20

    with pytest.raises(ValueError, match="overlap"):
        PolicySession(Model(), draws=4, select="coherent")
    with pytest.raises(ValueError, match="decay"):
        PolicySession(Model(), draws=4, advance=5, select="coherent", coherence_decay=0.0)
    with pytest.raises(ValueError, match="contrast"):
        PolicySession(Model(), draws=4, advance=5, select="coherent", contrast=-1.0)


def _brute(x, prev, shift, w, lam, robots):
    Cn, G, T, J = x.shape
    R = T - shift
    want = np.zeros((Cn, G))
    plan = np.zeros(Cn, dtype=bool)
    for c in range(Cn):
        p = prev[robots[c] if robots is not None else c]
        coh, med = [0.0] * G, [0.0] * G
        for g in range(G):
            for tau in range(R):
                for j in range(J):
                    pv, wt = float(p[tau + shift, j]), float(w[tau])
                    if math.isnan(pv) or wt == 0.0:
                        continue
                    plan[c] = True
                    coh[g] += wt * (float(x[c, g, tau, j]) - pv) ** 2
            for k in range(G):
                for t in range(T):
                    for j in range(J):
                        med[g] += (float(x[c, g, t, j]) - float(x[c, k, t, j])) ** 2
        for g in range(G):
            want[c, g] = coh[g] + lam * med[g] if plan[c] else med[g]
    return want, plan


@pytest.mark.parametrize("lam", [0.0, 0.37])
@pytest.mark.parametrize("G", [1, 2, 5, 9])
def test_coherent_ref_against_a_brute_force_loop(G, lam):
    rng = np.random.default_rng(300 + G)
    Cn, T, J, S = 4, 4, 5, 1
    x = rng.standard_normal((Cn, G, T, J)).astype(np.float32)
    prev = rng.standard_normal((Cn + 1, T, J)).astype(np.float32)
    prev[1, 2] = np.nan                       # a NaN row
    prev[2] = np.nan                          # an all-NaN plan: the medoid's scores
    prev[3, 0] = np.nan                       # a NaN outside the overlap changes nothing
    w = np.array([1.0, 0.0, 0.25, 7.0], dtype=np.float32)     # a zero weight; w[3] is beyond R and never read
    for robots in (None, [4, 2, 0, 1]):
        pv = prev[:Cn] if robots is None else prev
        want, plan = _brute(x, pv, S, w, lam, robots)
        np.testing.assert_allclose(coherent_ref.costs(x, G, pv, S, w, lam, robots), want, rtol=1e-12, atol=0)
        assert coherent_ref.has_plan(x, G, pv, S, w, robots).tolist() == plan.tolist()
        assert plan.tolist() == ([True, True, False, True] if robots is None else [True, False, True, True])
        pick = [min(range(G), key=lambda g: (want[c, g], g)) for c in range(Cn)]
        assert coherent_ref.choose(x, G, pv, S, w, lam, robots).tolist() == pick
        assert coherent_ref.choose(x.reshape(Cn * G, T, J), G, pv, S, w, lam, robots).tolist() == pick
        if G == 1:
            assert pick == [0] * Cn and np.isinf(coherent_ref.margins(x, G, pv, S, w, lam, robots)).all()
    wild = prev[:Cn].copy()
    wild[:, S + 1] = 1e6                      # the row that meets the zero weight
    np.testing.assert_array_equal(coherent_ref.costs(x, G, wild, S, w, lam), coherent_ref.costs(x, G, prev[:Cn], S, w, lam))


def test_coherent_ref_ties_go_to_the_lowest_index():
    rng = np.random.default_rng(8)
    x = rng.standard_normal((1, 5, 4, 5)).astype(np.float32) * 10
    prev = rng.standard_normal((1, 4, 5)).astype(np.float32)
    x[0, 1, :3] = prev[0, 1:] + 0.01
    x[0, 3] = x[0, 1]
    w = np.ones(4, dtype=np.float32)
    assert coherent_ref.choose(x, 5, prev, 1, w, 0.0).tolist() == [1] and coherent_ref.margins(x, 5, prev, 1, w, 0.0).tolist() == [0.0]


@pytest.mark.parametrize("decay", [0.5, 1.0, 0.9, 1 / 3])
def test_row_weights_are_float64_powers_rounded_once(decay):
    from soccerdiffusion_amd import ops

    T = 100
    w = ops.coherence_weights_host(T, decay)
    assert w.dtype == np.float32 and w.shape == (T,)
    want = np.array([np.float32(float(decay) ** tau) for tau in range(T)], dtype=np.float32)
    assert w.tobytes() == want.tobytes()
    assert w[0] == 1.0 and (w >= 0).all()


@pytest.mark.parametrize("contrast,shift,G,T,J,decay", [(1.0, 5, 8, 10, 20, 0.5), (0.3, 1, 5, 10, 20, 1.0), (2.0, 50, 3, 100, 32, 0.5),
                                                         (1.0, 1, 2, 3, 7, 0.9)])
def test_lam_is_float64_arithmetic_rounded_once(contrast, shift, G, T, J, decay):
    from soccerdiffusion_amd import ops

    w = ops.coherence_weights_host(T, decay)
    total = sum(float(v) for v in w[:T - shift])                 # the fp32 weights the kernel reads, summed in float64
    want = float(np.float32(contrast * (J * total) / ((G - 1) * T * J)))
    assert ops.coherence_lambda(contrast, w, shift, G, T, J) == want
    assert ops.coherence_lambda(contrast, w, shift, 1, T, J) == 0.0       # one draw: no second term
    assert ops.coherence_lambda(0.0, w, shift, G, T, J) == 0.0
    # contrast = 1 weighs the mean weighted square per overlap element against the mean square per medoid element, one to one
    lam = ops.coherence_lambda(1.0, w, shift, G, T, J)
    assert lam * ((G - 1) * T * J) == pytest.approx(J * total, rel=1e-6)


def test_cli_parses_select():
    from soccerdiffusion_amd.cli import _select_arg, build_parser

    ap = build_parser()
    a = ap.parse_args(["rollout", "c.pt", "--synthetic", "2"])
    assert (a.select, a.coherence_decay, a.contrast) == ("medoid", 0.5, 0.0)
    a = ap.parse_args(["rollout", "c.pt", "--synthetic", "2", "--draws", "4", "--advance", "5", "--select", "coherent", "--coherence-decay", "0.8",
                       "--contrast", "1.5"])
    assert (a.select, a.coherence_decay, a.contrast) == ("coherent", 0.8, 1.5)
    _select_arg(a, 10)
    with pytest.raises(SystemExit):
        ap.parse_args(["rollout", "c.pt", "--select", "mean"])
    for extra, word in ((["--coherence-decay", "0"], "decay"), (["--contrast", "-1"], "contrast"), (["--advance", "10"], "overlap")):
        bad = ap.parse_args(["rollout", "c.pt", "--synthetic", "2", "--draws", "4", "--advance", "5", "--select", "coherent", *extra])
        with pytest.raises(SystemExit, match=word):
            _select_arg(bad, 10)
    no_overlap = ap.parse_args(["rollout", "c.pt", "--synthetic", "2", "--draws", "4", "--select", "coherent"])
    with pytest.raises(SystemExit, match="overlap"):
        _select_arg(no_overlap, 10)


def test_plan_change_rms_on_a_hand_made_pair_of_ticks():
    from soccerdiffusion_amd.cli import plan_change_rms

    K, N, T, J, S = 2, 1, 4, 2, 1
    pub = torch.zeros(K, N, T, J)
    pub[0, 0] = torch.tensor([[9.0, 9.0], [1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    pub[1, 0] = torch.tensor([[1.0, 2.0], [3.0, 5.0], [7.0, 6.0], [-8.0, -8.0]])      # rows 0 .. 2 meet rows 1 .. 3 of the tick before
    # differences over the three overlapping rows: (0, 0), (0, 1), (2, 0): mean square 5 / 6
    assert plan_change_rms(pub, S) == pytest.approx(math.sqrt(5.0 / 6.0), rel=1e-12)
    assert plan_change_rms(torch.cat([pub, pub[1:]]), 0) == pytest.approx(math.sqrt(((pub[1] - pub[0]) ** 2).mean().item() / 2), rel=1e-6)
    assert math.isnan(plan_change_rms(pub[:1], S)) and math.isnan(plan_change_rms(pub, T))
    # a robot that was reset after the first tick starts a new episode: nothing left to compare
    assert math.isnan(plan_change_rms(pub, S, resets=torch.tensor([[True], [False]])))
    two = torch.cat([pub, pub + 100.0], dim=1)
    assert plan_change_rms(two, S, resets=torch.tensor([[False, True], [False, False]])) == pytest.approx(math.sqrt(5.0 / 6.0), rel=1e-12)
