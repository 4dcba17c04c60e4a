"""What a captured session tick needs to stay valid for as long as it can be replayed, and to be destroyed at a permitted moment: a
graphed session is freed by its reference count and captures with Python's collector off; and a scratch buffer of ops.workspace that
is outgrown while a graph is being captured stays alive, because an earlier call of the same capture has put its address into the graph
(the context encoders, then the rollout)."""

import gc
import weakref

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_a_dropped_graphed_session_dies_by_its_reference_count_and_no_collection_runs_inside_a_capture(monkeypatch):
    """A session and its captured tick are no reference cycle: dropping the session destroys the graph there and then, not whenever the
    collector next runs - which may be inside a later capture, where destroying a graph is not permitted.  And the capture itself runs
    with the collector off, whoever else left a dead graph behind."""
    from test_gpu_session import TINY, _synthetic_model

    from soccerdiffusion_amd import session as sess

    model = _synthetic_model({**TINY, "trajectory_prediction_length": 10})[0]
    seen = []
    real = sess._GraphedTick._run
    monkeypatch.setattr(sess._GraphedTick, "_run", lambda self: (seen.append((torch.cuda.is_current_stream_capturing(), gc.isenabled())), real(self))[1])
    assert gc.isenabled()
    s = sess.PolicySession(model, num_inference_steps=3, batch=2, use_graph=True)
    g = torch.Generator().manual_seed(5)
    s.push_joint_state(((torch.rand(2, 5, 20, generator=g) - 0.5) * 6).cuda())
    traj = s.step()
    torch.cuda.synchronize()
    assert torch.isfinite(traj).all()
    assert seen == [(False, True), (True, False)] and gc.isenabled()      # the warm-up, then the capture with the collector off
    tick = weakref.ref(s._graph)
    gc.disable()
    try:
        del s
        assert tick() is None      # freed by the reference count alone
    finally:
        gc.enable()


def test_a_workspace_outgrown_during_capture_stays_alive():
    from soccerdiffusion_amd import ops

    # eager: grow-only, and the outgrown buffer is simply dropped (the stream's order protects the kernels already queued)
    first = ops.workspace(1024, "cuda")
    retired = len(ops._ws_retired)
    bigger = ops.workspace(first.numel() + 1024, "cuda")
    assert bigger.numel() >= first.numel() + 1024 and len(ops._ws_retired) == retired
    assert ops.workspace(16, "cuda") is bigger
    # capturing: the buffer an earlier call of the capture was given survives the later, larger request
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        small = ops.workspace(1024, "cuda")
        small[:4].add_(1.0)                                  # its address is in the graph now
        large = ops.workspace(small.numel() + 4096, "cuda")
        large[:4].add_(1.0)
    assert large is not small and large.numel() >= small.numel() + 4096
    assert any(r is small for r in ops._ws_retired)
    assert len(ops._ws_retired) == retired + 1
