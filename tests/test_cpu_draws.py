"""Several draws per observation (sd_ddim_sample_draws, sd_select_medoid, PolicySession(draws=...)): everything that needs no GPU - the
symbols, the argument errors raised before any launch, the fp64 medoid reference against a brute-force loop, the command line, and the
plan's size limit, which counts contexts."""

import ctypes as C

import numpy as np
import pytest
import torch

import draws_ref


def test_symbols_resolve_in_the_library_and_in_lib_py():
    from soccerdiffusion_amd import _lib

    lib = _lib.load()
    for name in ("sd_ddim_sample_draws", "sd_select_medoid", "sd_sampler_route_draws"):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes is not None, name
    assert len(lib.sd_ddim_sample_draws.argtypes) == 19 and len(lib.sd_select_medoid.argtypes) == 8
    assert lib.sd_abi_version() == 1   # additive: the version stays


def _weights():
    from soccerdiffusion_amd import _lib

    w = _lib.DenoiserWeights()
    return w


@pytest.mark.parametrize("B,draws", [(6, 0), (6, -2), (6, 4), (7, 2)])
def test_bad_group_sizes_are_refused_before_any_launch(B, draws):
    """draws < 1 and B % draws != 0: SD_E_BADARG ahead of every other check (the weights here are an all-NULL struct, the pointers NULL)."""
    from soccerdiffusion_amd import _lib

    lib = _lib.load()
    rc = lib.sd_ddim_sample_draws(C.byref(_weights()), None, None, None, None, None, None, None, B, 10, 9, 3, None, -1, None, None, None, draws, None)
    assert rc == -1, rc   # SD_E_BADARG
    assert b"draws" in lib.sd_last_error()


@pytest.mark.parametrize("given", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)])
def test_partial_pin_pointers_are_refused_before_any_launch(given):
    from soccerdiffusion_amd import _lib

    lib = _lib.load()
    buf = (C.c_float * 4)()
    pins = [C.cast(buf, C.c_void_p) if g else None for g in given]
    rc = lib.sd_ddim_sample_draws(C.byref(_weights()), None, None, None, None, None, None, None, 6, 10, 9, 3, None, -1, *pins, 2, None)
    assert rc == -1, rc
    assert b"pin" in lib.sd_last_error()


def test_select_medoid_argument_errors():
    from soccerdiffusion_amd import _lib

    lib = _lib.load()
    buf = C.cast((C.c_float * 4)(), C.c_void_p)
    for Cn, G, T, J in ((0, 2, 10, 20), (2, 0, 10, 20), (2, 65, 10, 20), (2, 2, 0, 20), (2, 2, 10, 0)):
        assert lib.sd_select_medoid(buf, buf, None, Cn, G, T, J, None) == -1, (Cn, G, T, J)
    assert lib.sd_select_medoid(None, buf, None, 2, 2, 10, 20, None) == -1
    assert lib.sd_select_medoid(buf, None, None, 2, 2, 10, 20, None) == -1
    assert lib.sd_select_medoid(buf, buf, buf, 2, 2, 10, 20, None) == -1   # out must not alias x


def test_ops_shape_errors_come_before_any_device_check():
    """Context / noise mismatch, draws < 1, B % draws: ValueError from CPU tensors - nothing reached a launch (a CPU tensor that got as far
    as the device check would raise RuntimeError)."""
    from soccerdiffusion_amd import ops

    x = torch.zeros(6, 10, 20)
    toks, coef = torch.zeros(3, 256), np.zeros((3, 4), np.float32)
    with pytest.raises(ValueError, match="context"):
        ops.ddim_sample(None, torch.zeros(2, 9, 256), toks, coef, x, draws=2)      # 2 contexts x 2 draws != 6
    with pytest.raises(ValueError, match="context"):
        ops.ddim_sample(None, torch.zeros(6, 9, 256), toks, coef, x, draws=3)      # the repeated context is not what draws takes
    with pytest.raises(ValueError, match="multiple"):
        ops.ddim_sample(None, None, toks, coef, x, draws=4)
    for bad in (0, -1, True, 2.0):
        with pytest.raises(ValueError, match="draws"):
            ops.ddim_sample(None, torch.zeros(3, 9, 256), toks, coef, x, draws=bad)
    with pytest.raises(ValueError, match="context"):
        ops.ddim_sample_guarded(None, torch.zeros(2, 9, 256), toks, coef, x, draws=2)
    with pytest.raises(ValueError, match="draws"):
        ops.select_medoid(torch.zeros(6, 10, 20), 65)
    with pytest.raises(ValueError, match="draws"):
        ops.GraphedSampler(None, 6, 10, 9, toks, coef, draws=4)


def test_distilled_decoder_takes_no_draws():
    from soccerdiffusion_amd.session import PolicySession

    assert PolicySession.check_draws(1, "medoid", True) == (1, "medoid")
    assert PolicySession.check_draws(8, "medoid", False) == (8, "medoid")
    with pytest.raises(ValueError, match="distilled"):
        PolicySession.check_draws(2, "medoid", True)
    for bad in (0, 65, True, 2.5):
        with pytest.raises(ValueError, match="draws"):
            PolicySession.check_draws(bad)
    with pytest.raises(ValueError, match="select"):
        PolicySession.check_draws(2, "mean")

    class Model:   # the constructor validates before it looks at a device: no parameters are touched
        trajectory_prediction_length = 10

    with pytest.raises(ValueError, match="distilled"):
        PolicySession(Model(), draws=2, distilled=True)


@pytest.mark.parametrize("G", [1, 2, 5, 9])
def test_draws_ref_against_a_brute_force_loop(G):
    rng = np.random.default_rng(100 + G)
    Cn, T, J = 3, 4, 5
    x = rng.standard_normal((Cn, G, T, J)).astype(np.float32)
    want_scores = np.zeros((Cn, G))
    for c in range(Cn):
        for i in range(G):
            for k in range(G):
                for t in range(T):
                    for j in range(J):
                        want_scores[c, i] += (float(x[c, i, t, j]) - float(x[c, k, t, j])) ** 2
    want = [min(range(G), key=lambda i: (want_scores[c, i], i)) for c in range(Cn)]
    np.testing.assert_allclose(draws_ref.scores(x, G), want_scores, rtol=1e-12, atol=0)
    assert draws_ref.medoid(x, G).tolist() == want
    assert draws_ref.medoid(x.reshape(Cn * G, T, J), G).tolist() == want   # the flat layout the sampler returns
    if G == 1:
        assert draws_ref.medoid(x, G).tolist() == [0] * Cn and np.isinf(draws_ref.margins(x, G)).all()


def test_draws_ref_ties_go_to_the_lowest_index():
    rng = np.random.default_rng(7)
    x = rng.standard_normal((1, 5, 4, 5)).astype(np.float32) * 10
    x[0, 1] = 0.01 * rng.standard_normal((4, 5)).astype(np.float32)
    x[0, 3] = x[0, 1]
    assert draws_ref.medoid(x, 5).tolist() == [1] and draws_ref.margins(x, 5).tolist() == [0.0]


def test_cli_parses_draws():
    from soccerdiffusion_amd.cli import build_parser

    ap = build_parser()
    assert ap.parse_args(["sample", "c.pt"]).draws == 1
    assert ap.parse_args(["sample", "c.pt", "--draws", "3", "--num_samples", "4"]).draws == 3
    assert ap.parse_args(["rollout", "c.pt", "--synthetic", "2"]).draws == 1
    assert ap.parse_args(["rollout", "c.pt", "--synthetic", "2", "--draws", "8", "--carry", "3"]).draws == 8
    for bad in ("0", "65", "x"):
        with pytest.raises(SystemExit):
            ap.parse_args(["sample", "c.pt", "--draws", bad])


def test_the_size_limit_of_the_tuned_kernels_counts_contexts():
    """d = 256, Mk = 11: C * Mk * 2 d < 2^30 <= C * G * Mk * 2 d at C = 100 000, G = 2.  The shared call keeps the tuned route, whose folded
    blocks exist once per context; the same 200 000 trajectories with a context each do not fit it.  sd_sampler_route's answers stay."""
    from soccerdiffusion_amd import _lib

    d, heads, T, Mc, J, L, Cn, G = 256, 4, 100, 10, 20, 4, 100_000, 2
    assert Cn * (Mc + 1) * 2 * d < 2 ** 30 <= Cn * G * (Mc + 1) * 2 * d
    assert _lib.sampler_route(d, heads, T, Mc, J, L, Cn) == "TRAJ_TUNED"
    assert _lib.sampler_route(d, heads, T, Mc, J, L, Cn * G) == "TRAJ_GENERIC"
    assert _lib.sampler_route_draws(d, heads, T, Mc, J, L, Cn * G, G) == "TRAJ_TUNED"
    assert _lib.sampler_route_draws(d, heads, T, Mc, J, L, Cn * G, 1) == "TRAJ_GENERIC"
    assert _lib.sampler_route_draws(d, heads, T, Mc, J, L, Cn * G, G, max_mode=4) == "TRAJ_TUNED_2P"
    assert _lib.sampler_route_draws(d, heads, T, 0, J, L, Cn * G * 8, G) == _lib.sampler_route(d, heads, T, 0, J, L, Cn * G * 8)   # no context: nothing shared
    # everything else is a function of the same integers: a table of shapes answers alike with and without a group size
    for dd, TT, MM, BB in ((256, 100, 10, 8), (256, 10, 20, 6), (128, 10, 30, 6), (512, 10, 5, 6), (64, 16, 13, 6), (256, 100, 80, 4)):
        for mode in (-1, 1, 2, 3, 4):
            assert _lib.sampler_route_draws(dd, heads, TT, MM, J, 2, BB, 2, mode) == _lib.sampler_route(dd, heads, TT, MM, J, 2, BB, mode), (dd, TT, MM, mode)
    lib = _lib.load()
    assert lib.sd_sampler_route_draws(d, heads, T, Mc, J, L, 7, 3, 2) == -1 and lib.sd_sampler_route_draws(d, heads, T, Mc, J, L, 6, 3, 0) == -1
