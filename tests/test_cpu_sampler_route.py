"""The sampler's kernel route (csrc/sd_sampler_plan.h, reported by sd_sampler_route / sd_sampler_mode) pinned for a table of shapes: the
smallest at which each route is still selected, both sides of every threshold, the shipped YAMLs' shapes, and the four A/B switches of
the environment.  No GPU: the library loads without a device and the two exports launch nothing."""

import itertools
import json
import os
import subprocess
import sys

import pytest

from conftest import REPO
from test_gpu_shipped_shapes_grade import SHIPPED

# d, heads, T, Mc, J, L, B, cap, route
TABLE = [
    (64, 4, 16, 10, 10, 2, 2, 3, "CHAINS_F32"),
    (128, 4, 16, 40, 8, 1, 2, 2, "CHAINS_F16"),
    (128, 4, 16, 40, 8, 1, 2, 1, "CHAINS_F32"),
    (128, 4, 16, 3, 8, 1, 2, 2, "FUSED"),
    (128, 4, 64, 3, 8, 1, 2, 2, "FUSED_FOLD"),
    (256, 4, 64, 3, 8, 1, 2, 2, "FUSED_FOLD_F16"),
    (256, 4, 64, 3, 8, 1, 2, 1, "FUSED_FOLD"),
    (256, 4, 64, 3, 8, 1, 2, 0, "FUSED"),
    (256, 4, 10, 3, 20, 2, 2, 3, "TRAJ_TUNED"),
    (256, 4, 10, 3, 20, 2, 2, 4, "TRAJ_TUNED_2P"),
    (256, 4, 10, 15, 20, 2, 2, 3, "TRAJ_TUNED"),          # 16 memory rows with the step row: one key tile
    (256, 4, 10, 16, 20, 2, 2, 3, "TRAJ_TUNED_WIDE"),
    (256, 4, 10, 16, 20, 2, 2, 4, "TRAJ_TUNED_WIDE"),     # no two-product wide kernel
    (256, 4, 10, 63, 20, 2, 2, 3, "TRAJ_TUNED_WIDE"),
    (256, 4, 10, 64, 20, 2, 2, 3, "TRAJ_GENERIC"),
    (256, 4, 100, 3, 20, 2, 2, 3, "TRAJ_TUNED"),
    (256, 4, 101, 3, 20, 2, 2, 3, "FUSED_FOLD_F16"),      # horizon beyond both families
    (128, 4, 10, 33, 22, 1, 2, 3, "TRAJ_GENERIC"),
    (512, 4, 48, 10, 20, 2, 2, 3, "TRAJ_GENERIC"),
    (512, 4, 49, 10, 20, 2, 2, 3, "FUSED"),
    (256, 4, 10, 3, 20, 9, 2, 3, "FUSED"),                # nine layers: sd_sampler_mode, which does not see them, stays 3
    (256, 4, 10, 3, 33, 2, 2, 3, "FUSED"),
    (256, 8, 16, 3, 8, 1, 2, 2, "CHAINS_F16"),
    (256, 4, 10, 63, 20, 2, 32768, 3, "TRAJ_GENERIC"),    # B * Mk * 2 d = 2^30 floats: the size limit refuses the tuned family
]
MODE = {"FUSED_FOLD": 1, "FUSED_FOLD_F16": 2, "TRAJ_TUNED": 3, "TRAJ_TUNED_2P": 3, "TRAJ_TUNED_WIDE": 3, "TRAJ_GENERIC": 3}   # every other route: 0
GRID = sorted({r[:5] for r in TABLE} | set(itertools.product((64, 128, 256, 512), (2, 4, 8), (1, 10, 16, 48, 49, 63, 64, 100, 101),
                                                             (0, 3, 15, 16, 63, 64, 311), (1, 20, 21, 32, 33))))


@pytest.fixture(scope="module")
def lib():
    from soccerdiffusion_amd import _lib, build

    build.build()
    return _lib


@pytest.mark.parametrize("row", TABLE, ids=lambda r: "-".join(map(str, r)))
def test_route_table(lib, row):
    assert lib.sampler_route(*row[:8]) == row[8]


def test_routes_mirror_the_header(lib):
    hdr = open(os.path.join(REPO, "include", "soccerdiffusion_hip.h")).read()
    for i, name in enumerate(lib.ROUTES):
        assert f"#define SD_ROUTE_{name} {i}\n" in hdr
    assert hdr.count("#define SD_ROUTE_") == len(lib.ROUTES)


def test_automatic_cap_is_three(lib):
    for row in TABLE:
        assert lib.sampler_route(*row[:7], -1) == lib.sampler_route(*row[:7], 3)


def test_nine_layers_leave_the_trajectory_kernels_but_not_sd_sampler_mode(lib):
    assert lib.load().sd_sampler_mode(256, 4, 10, 3, 20) == 3
    assert lib.sampler_route(256, 4, 10, 3, 20, 8, 2, 3) == "TRAJ_TUNED" and lib.sampler_route(256, 4, 10, 3, 20, 9, 2, 3) == "FUSED"


def test_shipped_yaml_shapes(lib):
    want = {(128, 311): "TRAJ_GENERIC", (512, 311): "TRAJ_GENERIC", (256, 50): "TRAJ_TUNED_WIDE", (256, 0): "TRAJ_TUNED", (256, 10): "TRAJ_TUNED"}
    seen = set()
    for d, T, Mc, _, L, B in SHIPPED:
        for J in (20, 22):
            assert lib.sampler_route(d, 4, T, Mc, J, L, B, 3) == want[d, Mc]
            assert lib.load().sd_sampler_mode(d, 4, T, Mc, J) == 3
        seen.add((d, Mc, L))
    assert len(seen) == 5


def test_sd_sampler_mode_is_the_mode_of_the_route_at_one_layer_one_trajectory(lib):
    h = lib.load()
    for d, heads, T, Mc, J in GRID:
        assert h.sd_sampler_mode(d, heads, T, Mc, J) == MODE.get(lib.sampler_route(d, heads, T, Mc, J, 1, 1, 3), 0), (d, heads, T, Mc, J)


# ---- the switches are read once per process: each in a fresh child that only loads the library and prints
CHILD = """import json, sys
from soccerdiffusion_amd import _lib
print(json.dumps([_lib.load().sd_sampler_route(*r) for r in json.loads(sys.argv[1])]))"""
SWITCH_ROWS = [r[:8] for r in TABLE] + [(256, 4, 10, 16, 20, 2, 2, 3), (256, 4, 10, 40, 20, 2, 2, 3)]


def _routes_under(env, rows=SWITCH_ROWS):
    from soccerdiffusion_amd._lib import ROUTES

    e = {k: v for k, v in os.environ.items() if not k.startswith("SD_")}
    e.update(env, PYTHONPATH=REPO)
    out = subprocess.run([sys.executable, "-c", CHILD, json.dumps(rows)], env=e, capture_output=True, text=True, check=True, cwd=REPO)
    return [ROUTES[r] if r >= 0 else r for r in json.loads(out.stdout.strip().splitlines()[-1])]


def test_a_cap_outside_minus_one_to_four_is_an_argument_error(lib):
    # (in a child: the error text it leaves is per process)
    assert _routes_under({}, [(256, 4, 10, 3, 20, 2, 2, 5), (256, 4, 10, 3, 20, 2, 2, -2), (256, 4, 10, 3, 20, 2, 2, 4)]) == [-1, -1, "TRAJ_TUNED_2P"]


@pytest.fixture(scope="module")
def plain(lib):
    got = _routes_under({})
    assert got[:len(TABLE)] == [r[8] for r in TABLE]
    return got


def test_switch_traj_off_removes_every_trajectory_route(lib, plain):
    got = _routes_under({"SD_SAMPLER_TRAJ": "0"})
    assert not any(g.startswith("TRAJ_") for g in got)
    assert all(g == p for g, p in zip(got, plain) if not p.startswith("TRAJ_"))
    assert got[SWITCH_ROWS.index((256, 4, 10, 3, 20, 2, 2, 3))] == "FUSED"   # (horizon 10: no fold)


def test_switch_gemm_f32_removes_every_trajectory_and_f16_route(lib, plain):
    got = _routes_under({"SD_SAMPLER_GEMM": "f32"})
    assert set(got) <= {"CHAINS_F32", "FUSED", "FUSED_FOLD"}
    assert all(g == p for g, p in zip(got, plain) if p in ("CHAINS_F32", "FUSED", "FUSED_FOLD"))
    assert got[SWITCH_ROWS.index((256, 4, 64, 3, 8, 1, 2, 2))] == "FUSED_FOLD" and got[SWITCH_ROWS.index((128, 4, 16, 40, 8, 1, 2, 2))] == "CHAINS_F32"


def test_switch_trajg_off_removes_only_the_generic_route(lib, plain):
    got = _routes_under({"SD_SAMPLER_TRAJG": "0"})
    assert "TRAJ_GENERIC" in plain and "TRAJ_GENERIC" not in got
    assert all(g == p for g, p in zip(got, plain) if p != "TRAJ_GENERIC")


def test_switch_maxrows_moves_the_wide_shapes_to_the_generic_kernels(lib, plain):
    got = _routes_under({"SD_TRAJ_MAXROWS": "16"})
    assert "TRAJ_TUNED_WIDE" in plain and "TRAJ_TUNED_WIDE" not in got
    assert all(g == ("TRAJ_GENERIC" if p == "TRAJ_TUNED_WIDE" else p) for g, p in zip(got, plain))
