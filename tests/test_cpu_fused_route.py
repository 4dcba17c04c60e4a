"""The rollout form of the sampler's plan (csrc/sd_sampler_plan.h, `SamplerPlan::rollout_fused`, asked through sd_sampler_route with
SD_ASK_ROLLOUT): fused - every DDIM step of a trajectory in one launch - exactly for a plain rollout on the tuned one-key-tile trajectory
routes, one launch per step for everything else, and for everything under SD_TRAJ_ROLLOUT=steps.  No GPU: the library loads without a
device and the export launches nothing."""

import json
import os
import subprocess
import sys

import pytest

from conftest import REPO
from test_cpu_sampler_route import TABLE

FUSED_ROUTES = ("TRAJ_TUNED", "TRAJ_TUNED_2P")
KINDS = ({}, {"trace": True}, {"pin": True}, {"loop": True}, {"trace": True, "pin": True})


@pytest.fixture(scope="module")
def lib():
    from soccerdiffusion_amd import _lib, build

    build.build()
    return _lib


@pytest.mark.parametrize("row", TABLE, ids=lambda r: "-".join(map(str, r)))
def test_fused_exactly_for_plain_rollouts_on_the_tuned_routes(lib, row):
    route = lib.sampler_route(*row[:8])
    assert route == row[8]
    for kind in KINDS:
        want = "FUSED" if (not kind and route in FUSED_ROUTES) else "PER_STEP"
        assert lib.sampler_rollout(*row[:8], **kind) == want, (row, kind)


def test_every_route_is_covered(lib):
    assert {r[8] for r in TABLE} == set(lib.ROUTES)
    assert {r[8] for r in TABLE if r[7] < 3} == {"CHAINS_F32", "CHAINS_F16", "FUSED", "FUSED_FOLD", "FUSED_FOLD_F16"}   # modes 0 - 2


def test_a_pinned_call_at_cap_four_is_read_as_three(lib):
    # sd_ddim_sample_pin runs the mode-3 kernels at cap 4: still one launch per step
    assert lib.sampler_rollout(256, 4, 10, 3, 20, 2, 2, 4) == "FUSED" and lib.sampler_rollout(256, 4, 10, 3, 20, 2, 2, 4, pin=True) == "PER_STEP"


def test_the_automatic_cap_and_the_benchmark_shape(lib):
    assert lib.sampler_rollout(256, 4, 100, 10, 20, 4, 4096) == "FUSED" and lib.sampler_rollout(256, 4, 100, 10, 20, 4, 4096, 4) == "FUSED"
    assert lib.sampler_rollout(256, 4, 100, 10, 20, 4, 4096, 2) == "PER_STEP"


def test_asking_leaves_the_route_report_alone(lib):
    h = lib.load()
    assert h.sd_sampler_route(256, 4, 10, 3, 20, 2, 2, 3) == lib.ROUTES.index("TRAJ_TUNED")
    assert h.sd_sampler_route(256, 4, 10, 3, 20, 2, 2, 0x100 + 3) == 1 and h.sd_sampler_route(256, 4, 10, 3, 20, 2, 2, 0x100 + 0x10 + 3) == 0


CHILD = """import json, sys
from soccerdiffusion_amd import _lib
rows = json.loads(sys.argv[1])
print(json.dumps([[_lib.sampler_route(*r), _lib.sampler_rollout(*r)] for r in rows]))"""


def test_switch_forces_one_launch_per_step_and_moves_no_route(lib):
    rows = [r[:8] for r in TABLE]
    env = {k: v for k, v in os.environ.items() if not k.startswith("SD_")}
    env.update(SD_TRAJ_ROLLOUT="steps", PYTHONPATH=REPO)
    out = subprocess.run([sys.executable, "-c", CHILD, json.dumps(rows)], env=env, capture_output=True, text=True, check=True, cwd=REPO)
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert [g[0] for g in got] == [r[8] for r in TABLE]
    assert all(g[1] == "PER_STEP" for g in got)
    # ... and a cap outside 0 .. 4 stays an argument error when asked this way (in the child: the error text is per process)
    bad = subprocess.run([sys.executable, "-c", "import sys\nfrom soccerdiffusion_amd import _lib\nprint(_lib.load().sd_sampler_route(256, 4, 10, 3, 20, 2, 2, 0x100 + 5))"],
                         env=env, capture_output=True, text=True, check=True, cwd=REPO)
    assert bad.stdout.strip().splitlines()[-1] == "-1"
