"""The training path's kernel route (training.train_route) against the three predicates it replaced, written out here as one plain table
function over the same facts, on a grid that holds both sides of every threshold and every switch; and the two switches occur in that
one function only.  No GPU: the shape rule of sd_train_layer_fwd is injected (the library's own answer is compared where it loads)."""

import ast
import itertools
import os

import pytest

from conftest import REPO

D, HEADS, TS, MS, JS = (64, 128, 256, 512), (4, 8), (1, 10, 100, 101), (0, 1, 16, 17), (3, 4, 20, 22, 32, 36)
BOOLS = (False, True)


def layer_fwd_ok(d, heads, T, M):
    return d == 256 and heads == 4 and 1 <= T <= 100 and 1 <= M <= 16


def parent_rule(fused_on, traj_on, decoder, d, heads, T, M, J, ffn_is_d, params_ok, block_planes, traj_planes, x_differentiable):
    """(_fused_ok, _embed_head_ok, _traj_layer_weights is not None) of the code before train_route, fact by fact."""
    fused_ok = fused_on and d in (64, 128, 256) and params_ok and ffn_is_d and block_planes
    if not fused_ok:
        return "per_op", False, False
    embed_head_ok = (decoder and traj_on and not x_differentiable and d == 256 and J % 4 == 0 and 4 <= J <= 32 and T <= 100 and heads == 4
                     and traj_planes)
    traj_layer = decoder and traj_on and M > 0 and layer_fwd_ok(d, heads, T, M) and traj_planes
    return "chains", embed_head_ok, traj_layer


@pytest.mark.parametrize("fused_on,traj_on", list(itertools.product(BOOLS, BOOLS)), ids=lambda v: str(int(v)))
def test_route_equals_the_parent_predicates_over_the_grid(monkeypatch, fused_on, traj_on):
    from soccerdiffusion_amd import training

    monkeypatch.setenv("SD_TRAIN_FUSED", "1" if fused_on else "0")
    monkeypatch.setenv("SD_TRAIN_TRAJ", "1" if traj_on else "0")
    seen = set()
    for d, heads, T, M, J, bp, tp, ffn, xd in itertools.product(D, HEADS, TS, MS, JS, BOOLS, BOOLS, BOOLS, BOOLS):
        for decoder, params_ok in itertools.product(BOOLS, BOOLS):   # (the callers pair decoder with M > 0; the rule holds for any pairing)
            facts = dict(decoder=decoder, d=d, heads=heads, T=T, M=M, J=J, ffn_is_d=ffn, params_ok=params_ok, block_planes=bp, traj_planes=tp,
                         x_differentiable=xd)
            got = training.train_route(**facts, layer_fwd_ok=layer_fwd_ok)
            assert tuple(got) == parent_rule(fused_on, traj_on, **facts), facts
            assert got.stack in ("per_op", "chains") and (got.stack == "chains" or not (got.embed_head or got.traj_layers))
            seen.add(tuple(got))
    if fused_on and traj_on:   # the flags are independent: all four combinations occur, e.g. head without layers at 17 memory rows
        assert seen == {("per_op", False, False)} | {("chains", a, b) for a in BOOLS for b in BOOLS}
        edge = dict(decoder=True, d=256, heads=4, T=10, J=20, ffn_is_d=True, params_ok=True, block_planes=True, traj_planes=True, x_differentiable=False)
        assert tuple(training.train_route(M=16, **edge, layer_fwd_ok=layer_fwd_ok)) == ("chains", True, True)
        assert tuple(training.train_route(M=17, **edge, layer_fwd_ok=layer_fwd_ok)) == ("chains", True, False)
    elif fused_on:
        assert seen == {("per_op", False, False), ("chains", False, False)}
    else:
        assert seen == {("per_op", False, False)}


def test_switches_default_to_on(monkeypatch):
    from soccerdiffusion_amd import training

    monkeypatch.delenv("SD_TRAIN_FUSED", raising=False)
    monkeypatch.delenv("SD_TRAIN_TRAJ", raising=False)
    got = training.train_route(decoder=True, d=256, heads=4, T=10, M=11, J=20, ffn_is_d=True, params_ok=True, block_planes=True, traj_planes=True,
                               x_differentiable=False, layer_fwd_ok=layer_fwd_ok)
    assert tuple(got) == ("chains", True, True)


def test_injected_shape_rule_is_the_librarys():
    from soccerdiffusion_amd import build, ops

    build.build()
    for d, heads, T, M in itertools.product(D, HEADS, (0,) + TS, MS + (-1,)):
        assert ops.train_layer_fwd_ok(d, heads, T, M) == layer_fwd_ok(d, heads, T, M), (d, heads, T, M)


def _occurrences(tree, word):
    """Names of the functions (module level: '<module>') in whose code ``word`` occurs inside a string constant, docstrings aside."""
    docs = {id(n.body[0].value) for n in ast.walk(tree)
            if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef, ast.Module)) and n.body and isinstance(n.body[0], ast.Expr)
            and isinstance(n.body[0].value, ast.Constant) and isinstance(n.body[0].value.value, str)}
    found = []

    def walk(node, owner):
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
            owner = node.name
        if isinstance(node, ast.Constant) and isinstance(node.value, str) and word in node.value and id(node) not in docs:
            found.append(owner)
        for child in ast.iter_child_nodes(node):
            walk(child, owner)

    walk(tree, "<module>")
    return found


@pytest.mark.parametrize("switch", ["SD_TRAIN_FUSED", "SD_TRAIN_TRAJ"])
def test_each_switch_is_read_in_one_function_of_the_package(switch):
    pkg = os.path.join(REPO, "soccerdiffusion_amd")
    where = []
    for root, _, files in os.walk(pkg):
        for name in sorted(files):
            if name.endswith(".py"):
                path = os.path.join(root, name)
                where += [(os.path.relpath(path, pkg), fn) for fn in _occurrences(ast.parse(open(path).read()), switch)]
    assert where == [("training.py", "train_route")], where
