"""group_rank_k and lambdarank_grad_k on MI355X against the float64 oracle
of lambdarank_cases, per cell within (m + 12 + X) * 2^-23 * S + 1e-37
(lambdarank_cases.cell_bound has the derivation); LambdarankObjective and
ndcg_at on device tensors; the ranker end to end on the GPU."""
import numpy as np
import pytest
import torch

from mmlspark_amd.models.gbdt import ranking
from mmlspark_amd.models.gbdt.objectives import LambdarankObjective
from mmlspark_amd.ops import backend

from . import lambdarank_cases as lc

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs ROCm GPU")


def _run_ops(name):
    score, offsets, gid, label, gain, disc, inv = lc.op_inputs(name, "cuda")
    rank, rec = backend.group_rank(score, offsets, gid, label, gain, disc)
    g, h = backend.lambdarank_grad(rec, offsets, gid, inv,
                                   lc.case(name)["sigma"])
    return rank, rec, g, h


@requires_gpu
@pytest.mark.parametrize("name", lc.CASE_NAMES)
def test_group_rank_is_exactly_the_oracles(name):
    score, offsets, gid, label, gain, disc, _ = lc.op_inputs(name, "cuda")
    rank, rec = backend.group_rank(score, offsets, gid, label, gain, disc)
    assert rank.is_cuda and rank.dtype == torch.int32
    assert rank.shape == score.shape
    assert np.array_equal(rank.cpu().numpy(), lc.oracle(name)["rank"])
    assert rec.dtype == torch.float32 and rec.shape == (score.numel(), 4)
    want = torch.stack([score, label, gain, disc[rank.long()]], dim=1)
    assert torch.equal(rec, want)


@requires_gpu
@pytest.mark.parametrize("name", lc.CASE_NAMES)
def test_lambdarank_grad_within_bound_and_repeatable(name):
    _, _, g, h = _run_ops(name)
    assert g.is_cuda and g.dtype == torch.float32 and h.dtype == torch.float32
    worst = lc.check_grads(g.cpu().numpy(), h.cpu().numpy(), name, "gfx950")
    print(f"{name}: worst ratio to the bound {worst:.3f}")
    _, _, g2, h2 = _run_ops(name)
    assert torch.equal(g, g2) and torch.equal(h, h2)  # bit-identical


@requires_gpu
def test_ranks_stay_in_range_for_any_scores():
    """rank is a count: NaN and infinite scores cannot push it out of
    [0, m), so nothing downstream indexes out of bounds."""
    score, offsets, gid, label, gain, disc, inv = lc.op_inputs(
        "mixed-1-3", "cuda")
    score = score.clone()
    score[::5] = float("nan")
    score[1::11] = float("inf")
    score[2::13] = float("-inf")
    rank, rec = backend.group_rank(score, offsets, gid, label, gain, disc)
    m = torch.from_numpy(lc.oracle("mixed-1-3")["m"]).to("cuda")
    assert bool(((rank >= 0) & (rank < m)).all())
    g, h = backend.lambdarank_grad(rec, offsets, gid, inv, 1.0)
    assert g.shape == score.shape and h.shape == score.shape


def _objective(name):
    c = lc.case(name)
    obj = LambdarankObjective(sigmoid=c["sigma"], label_gain=c["label_gain"])
    obj.group_sizes = torch.from_numpy(c["sizes"])
    preds = torch.from_numpy(c["score"]).to("cuda").unsqueeze(-1)
    label = torch.from_numpy(c["label"]).to("cuda")
    return obj, preds, label


@requires_gpu
@pytest.mark.parametrize("name", ["mixed-2-8", "table", "empty"])
def test_objective_on_device_tensors(name, monkeypatch):
    monkeypatch.delenv("MMLSPARK_AMD_LAMBDARANK", raising=False)
    obj, preds, label = _objective(name)
    n = preds.shape[0]
    g, h = obj.grad_hess(preds, label, None)
    for t in (g, h):
        assert t.is_cuda and t.dtype == torch.float32 and t.shape == (n, 1)
    assert bool((h >= 1e-16).all())
    # the objective's own per-fit inputs feed the kernels: same bound on g;
    # h is the kernel's, clamped
    lc.check_grads(g.squeeze(-1).cpu().numpy(), None, name, "objective")
    inp = obj._device_inputs(label, preds.device)
    _, rec = backend.group_rank(preds.reshape(-1), inp.offsets, inp.gid,
                                inp.label, inp.gain, inp.disc_tbl)
    _, h_raw = backend.lambdarank_grad(rec, inp.offsets, inp.gid,
                                       inp.inv_idcg, obj.sigmoid)
    assert torch.equal(h.squeeze(-1), h_raw.clamp_min(1e-16))
    w = torch.linspace(0.5, 2.0, n, device="cuda")
    gw, hw = obj.grad_hess(preds, label, w)
    assert torch.equal(gw, g * w.unsqueeze(-1))
    assert torch.equal(hw, h * w.unsqueeze(-1))


@requires_gpu
def test_switch_off_runs_the_loop_and_agrees(monkeypatch):
    obj, preds, label = _objective("mixed_no_ties")
    monkeypatch.setenv("MMLSPARK_AMD_LAMBDARANK", "1")
    g, h = obj.grad_hess(preds, label, None)
    monkeypatch.setenv("MMLSPARK_AMD_LAMBDARANK", "0")

    def boom(*a, **k):
        raise AssertionError("rank op called with the switch off")
    monkeypatch.setattr(backend, "group_rank", boom)
    monkeypatch.setattr(backend, "lambdarank_grad", boom)
    gl, hl = obj.grad_hess(preds, label, None)
    assert gl.is_cuda and gl.shape == g.shape
    err_g = float((gl - g).abs().max() / g.abs().max())
    err_h = float((hl - h).abs().max() / h.abs().max())
    print(f"loop vs kernels: g {err_g * 2 ** 23:.2f}, h {err_h * 2 ** 23:.2f} "
          "(units of 2^-23 * max)")
    assert err_g <= 2.0 ** -20
    assert err_h <= 2.0 ** -20


@requires_gpu
@pytest.mark.parametrize("label_gain", [None, (0, 1, 1, 7)])
def test_ndcg_at_on_device_equals_the_host_loop(label_gain):
    gains = list(label_gain) if label_gain else None
    score, label, sizes = lc.ndcg_case(label_gain)
    want = lc.host_loop_ndcg(score, label, sizes, lc.EVAL_AT, gains)
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    got = ranking.ndcg_at(torch.from_numpy(score).to("cuda"),
                          torch.from_numpy(label).to("cuda"),
                          torch.from_numpy(offsets).to("cuda"),
                          lc.EVAL_AT, gains)
    for k, v in zip(lc.EVAL_AT, got):
        assert abs(v - want[k]) <= lc.ndcg_bound(k, len(sizes), want[k]), \
            (k, v, want[k])


@requires_gpu
def test_ranker_end_to_end_on_the_gpu(monkeypatch):
    """test_gbdt.test_ranker_validation_ndcg_and_early_stopping with
    device="cuda": gradients from the kernels, NDCG from the device path.
    Every recorded ndcg@k is what ndcg_at gives on the host for the scores
    of that iteration's trees."""
    from mmlspark_amd.models.gbdt.estimators import LightGBMRanker
    monkeypatch.delenv("MMLSPARK_AMD_LAMBDARANK", raising=False)
    calls = []
    real = backend.lambdarank_grad
    monkeypatch.setattr(backend, "lambdarank_grad",
                        lambda *a: calls.append(1) or real(*a))
    df = lc.ranker_frame()
    m = LightGBMRanker(numIterations=60, numLeaves=15, learningRate=0.1,
                       groupCol="group", evalAt=[3, 5],
                       validationIndicatorCol="isVal",
                       earlyStoppingRound=8, device="cuda").fit(df)
    evals = m._training_stats.evals
    assert evals, "validation metrics must be recorded"
    assert len(calls) == len(evals)  # one kernel pair per iteration
    keys = set(evals[0]["valid_0"].keys())
    assert keys == {"ndcg@3", "ndcg@5"}, keys
    ndcgs = [e["valid_0"]["ndcg@3"] for e in evals]
    bi = m.booster.best_iteration
    assert bi >= 0
    assert ndcgs[bi] == max(ndcgs), (bi, ndcgs)  # higher-is-better tracked
    assert max(ndcgs) > 0.6

    val = df[df["isVal"]]
    Xv = torch.from_numpy(np.stack(val["features"].to_numpy())).to("cuda")
    yv = torch.from_numpy(val["label"].to_numpy(dtype=np.float32))
    sizes = val.groupby("group", sort=False).size().to_numpy()
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    ev = ranking.NdcgEvaluator(yv, offsets, [3, 5])
    for e in evals:
        raw = m.booster.predict_raw(Xv, 0, e["iteration"] + 1)
        host = ev(raw.squeeze(-1).cpu())
        for k, v in zip([3, 5], host):
            rec = e["valid_0"][f"ndcg@{k}"]
            assert lc.recorded_within(rec, v, lc.ndcg_bound(k, len(sizes), v)), \
                (e["iteration"], k, rec, v)
