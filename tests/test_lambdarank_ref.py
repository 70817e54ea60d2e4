"""CPU references of the rank ops, the host-side validation, the device-path
plumbing of LambdarankObjective and ndcg_at, all on CPU tensors, against the
float64 oracle of lambdarank_cases."""
import numpy as np
import pytest
import torch

from mmlspark_amd.models.gbdt import ranking
from mmlspark_amd.models.gbdt.objectives import LambdarankObjective
from mmlspark_amd.ops import backend, cpu_ref

from . import lambdarank_cases as lc


@pytest.mark.parametrize("name", lc.CASE_NAMES)
def test_group_rank_is_the_stable_descending_order(name):
    score, offsets, gid, label, gain, disc, _ = lc.op_inputs(name)
    rank, rec = cpu_ref.group_rank(score, offsets, gid, label, gain, disc)
    o = lc.oracle(name)
    assert rank.dtype == torch.int32 and rank.shape == score.shape
    assert np.array_equal(rank.numpy(), o["rank"])
    assert rec.shape == (score.numel(), 4) and rec.dtype == torch.float32
    want = torch.stack([score, label, gain, disc[rank.long()]], dim=1)
    assert torch.equal(rec, want)


def test_group_rank_ties_and_signed_zero():
    """0.0 and -0.0 are equal scores: index decides, as in a stable sort."""
    s = np.array([1.0, 0.0, -0.0, 1.0, -0.0, 0.0, 2.0], dtype=np.float32)
    offsets = np.array([0, 7])
    want = lc.stable_ranks(s, offsets)
    assert want.tolist() == [1, 3, 4, 2, 5, 6, 0]
    z = torch.zeros(7)
    rank, _ = backend.group_rank(
        torch.from_numpy(s), torch.from_numpy(offsets),
        torch.zeros(7, dtype=torch.int32), z, z, z)
    assert rank.tolist() == want.tolist()


@pytest.mark.parametrize("name", lc.CASE_NAMES)
def test_lambdarank_grad_float32_within_bound(name):
    score, offsets, gid, label, gain, disc, inv = lc.op_inputs(name)
    _, rec = cpu_ref.group_rank(score, offsets, gid, label, gain, disc)
    g, h = backend.lambdarank_grad(rec, offsets, gid, inv,
                                   lc.case(name)["sigma"])
    assert g.dtype == torch.float32 and h.dtype == torch.float32
    worst = lc.check_grads(g.numpy(), h.numpy(), name, "cpu_ref f32")
    print(f"{name}: worst ratio to the bound {worst:.3f}")


def test_lambdarank_grad_is_generic_in_dtype():
    """The same code in float64 is the oracle's evaluation, to float64
    rounding: 2^-40 of the bound's scale leaves room for summation order."""
    name = lc.CASE_NAMES[0]
    args = lc.op_inputs(name, dtype=torch.float64)
    score, offsets, gid, label, gain, disc, inv = args
    _, rec = cpu_ref.group_rank(score, offsets, gid, label, gain, disc)
    assert rec.dtype == torch.float64
    g, h = cpu_ref.lambdarank_grad(rec, offsets, gid, inv, 1.0)
    o = lc.oracle(name)
    assert np.abs(g.numpy() - o["g"]).max() <= 2.0 ** -40 * o["S_g"].max()
    assert np.abs(h.numpy() - o["h"]).max() <= 2.0 ** -40 * o["S_h"].max()


def test_flat_and_table_cases_hit_what_they_are_for():
    o = lc.oracle("flat")
    assert (o["S_g"][:10] == 0).all() and (o["S_g"][10:] > 0).any()
    assert (o["X"] == 0).all()  # equal scores: x == 0 for every pair
    c, o = lc.case("table"), lc.oracle("table")
    # a document labelled 1 or 2 whose only differently-labelled partners
    # have the other of the two labels would be S == 0; at least the pairs
    # exist and the case has non-zero cells too
    assert {1.0, 2.0} <= set(c["label"].tolist())
    assert (o["S_g"] > 0).any()


def test_existing_loop_matches_the_oracle_semantically():
    """The per-group loop computes the same pairs, signs and discounts: on
    tie-free `mixed` it is within 2^-20 * max|g| of the oracle (measured
    1.3 * 2^-23 * max|g| and 2.4 * 2^-23 * max|h|; it rounds its own
    discounts and IDCG, so the kernel bound does not apply to it).  A wrong sign, a missing pair or a wrong
    discount shows at 2^-5 or more."""
    c, o = lc.case("mixed_no_ties"), lc.oracle("mixed_no_ties")
    obj = LambdarankObjective(sigmoid=c["sigma"])
    obj.group_sizes = torch.from_numpy(c["sizes"])
    g, h = obj.grad_hess(torch.from_numpy(c["score"]).unsqueeze(-1),
                         torch.from_numpy(c["label"]), None)
    g, h = g.squeeze(-1).numpy(), h.squeeze(-1).numpy()
    err_g = np.abs(g - o["g"]).max() / np.abs(o["g"]).max()
    err_h = np.abs(h - np.maximum(o["h"], 1e-16)).max() / o["h"].max()
    print(f"loop vs oracle: g {err_g * 2 ** 23:.2f}, h {err_h * 2 ** 23:.2f} "
          "(units of 2^-23 * max)")
    assert err_g <= 2.0 ** -20
    assert err_h <= 2.0 ** -20


# ------------------------------------------------------------ host validation
@pytest.mark.parametrize("offsets", [[1, 3, 5], [0, 3, 2, 5], [0, 3, 4],
                                     [0, 3, 6], []])
def test_bad_offsets_raise(offsets):
    with pytest.raises(ValueError):
        ranking.check_offsets(np.asarray(offsets, dtype=np.int64), 5)


@pytest.mark.parametrize("sizes", [[3, 3], [2, 2], [6, -1]])
def test_group_sizes_that_do_not_cover_the_labels_raise(sizes):
    obj = LambdarankObjective()
    obj.group_sizes = torch.tensor(sizes)
    with pytest.raises(ValueError):
        obj._device_inputs(torch.zeros(5), torch.device("cpu"))


@pytest.mark.parametrize("bad", [4.0, -1.0, 1.5, float("nan")])
def test_labels_outside_the_gain_table_raise(bad):
    obj = LambdarankObjective(label_gain=[0, 1, 1, 7])
    obj.group_sizes = torch.tensor([3])
    with pytest.raises(ValueError):
        obj._device_inputs(torch.tensor([0.0, bad, 3.0]),
                           torch.device("cpu"))
    with pytest.raises(ValueError):
        ranking.ndcg_at(torch.zeros(3), torch.tensor([0.0, bad, 3.0]),
                        np.array([0, 3]), [1], [0, 1, 1, 7])


# ------------------------------------------------------------ per-fit inputs
@pytest.mark.parametrize("name", lc.CASE_NAMES)
def test_per_fit_inputs_match_the_independent_tables(name):
    c, t = lc.case(name), lc.tables(name)
    obj = LambdarankObjective(sigmoid=c["sigma"], label_gain=c["label_gain"])
    obj.group_sizes = torch.from_numpy(c["sizes"])
    inp = obj._device_inputs(torch.from_numpy(c["label"]),
                             torch.device("cpu"))
    assert inp.offsets.dtype == torch.int64 and inp.gid.dtype == torch.int32
    assert np.array_equal(inp.offsets.numpy(), t["offsets"])
    assert np.array_equal(inp.gid.numpy(), t["gid"])
    assert np.array_equal(inp.gain.numpy(), t["gain"])
    assert np.array_equal(inp.disc_tbl.numpy(), t["disc_tbl"])
    # both sum the ideal DCG in float64 and round once: summation order only
    np.testing.assert_allclose(inp.inv_idcg.numpy(), t["inv_idcg"],
                               rtol=2.0 ** -23, atol=0)


def test_assigning_group_sizes_rebuilds_the_cache():
    """The two-batch numBatches shape: one objective, two sessions, each
    assigning its own groups."""
    obj = LambdarankObjective()
    label = torch.tensor([0.0, 1.0, 2.0, 1.0, 0.0, 2.0])
    dev = torch.device("cpu")
    obj.group_sizes = torch.tensor([2, 4])
    first = obj._device_inputs(label, dev)
    assert obj._device_inputs(label, dev) is first  # cached
    assert first.offsets.tolist() == [0, 2, 6]
    obj.group_sizes = torch.tensor([3, 3])
    second = obj._device_inputs(label, dev)
    assert second is not first
    assert second.offsets.tolist() == [0, 3, 6]
    assert second.gid.tolist() == [0, 0, 0, 1, 1, 1]
    # a changed label tensor rebuilds too: in place, or another tensor
    label[0] = 2.0
    third = obj._device_inputs(label, dev)
    assert third is not second and third.gain[0] == 3.0
    assert obj._device_inputs(label.clone(), dev) is not third


def test_cpu_tensors_keep_the_loop(monkeypatch):
    """grad_hess on CPU tensors never reaches the rank ops."""
    def boom(*a, **k):
        raise AssertionError("rank op called for CPU tensors")
    monkeypatch.setattr(backend, "group_rank", boom)
    monkeypatch.setattr(backend, "lambdarank_grad", boom)
    c = lc.case("flat")
    obj = LambdarankObjective()
    obj.group_sizes = torch.from_numpy(c["sizes"])
    g, h = obj.grad_hess(torch.from_numpy(c["score"]).unsqueeze(-1),
                         torch.from_numpy(c["label"]), None)
    assert g.shape == (22, 1) and (h >= 1e-16).all()


def test_switch_default_is_on(monkeypatch):
    monkeypatch.delenv("MMLSPARK_AMD_LAMBDARANK", raising=False)
    assert ranking.kernel_path_enabled()
    monkeypatch.setenv("MMLSPARK_AMD_LAMBDARANK", "0")
    assert not ranking.kernel_path_enabled()
    monkeypatch.setenv("MMLSPARK_AMD_LAMBDARANK", "1")
    assert ranking.kernel_path_enabled()


# ----------------------------------------------------------------------- NDCG
@pytest.mark.parametrize("label_gain", [None, (0, 1, 1, 7)])
def test_ndcg_at_equals_the_host_loop(label_gain):
    gains = list(label_gain) if label_gain else None
    score, label, sizes = lc.ndcg_case(label_gain)
    want = lc.host_loop_ndcg(score, label, sizes, lc.EVAL_AT, gains)
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    got = ranking.ndcg_at(torch.from_numpy(score), torch.from_numpy(label),
                          torch.from_numpy(offsets), lc.EVAL_AT, gains)
    assert len(got) == len(lc.EVAL_AT)
    for k, v in zip(lc.EVAL_AT, got):
        assert 0.0 < want[k] <= 1.0
        assert abs(v - want[k]) <= lc.ndcg_bound(k, len(sizes), want[k]), \
            (k, v, want[k])


def test_ndcg_at_without_documents_is_zero():
    got = ranking.ndcg_at(torch.zeros(0), torch.zeros(0), np.array([0, 0, 0]),
                          [1, 5])
    assert got == [0.0, 0.0]
    assert lc.host_loop_ndcg(np.zeros(0), np.zeros(0), [0, 0], [1, 5]) == \
        {1: 0.0, 5: 0.0}
