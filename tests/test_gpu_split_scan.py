"""split_scan_k + split_reduce_k (backend.split_scan) and sibling_scan_k
(backend.sibling_scan) on MI355X against the float64 oracle of
split_scan_cases: the exact (feature, bin) on every case, exact GL/HL/CL in
Family A, the measured bound in Family B; big = parent - small on every cell;
records bit-identical between the two entry points; and the argument checks
of both bindings, which raise before anything is launched."""
import numpy as np
import pytest
import torch

from mmlspark_amd.ops import backend

from . import split_scan_cases as sc

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs ROCm GPU")

DEAD = np.array([-np.inf, 0, 0, 0, 0, 0], dtype=np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@requires_gpu
@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_split_scan_names_the_oracles_split(name):
    out = sc.run(backend.split_scan, name, "cuda")
    worst = sc.check_result(out, name, *sc.tolerances(name))
    print("%s: gain error / scale %.3g, prefix error / sum %.3g"
          % ((name,) + worst))
    again = sc.run(backend.split_scan, name, "cuda")
    assert np.array_equal(_bits(out), _bits(again))       # bit-identical


def _sibling_inputs(name, wide):
    c = sc.cases()[name]
    sg, sh = sc.fixed_scales(name, wide)
    i_small, i_other = 0, (1 if c["hists"].shape[0] > 1 else 0)
    small = sc.fixed_hist(name, i_small, sg, sh).cuda()
    other = sc.fixed_hist(name, i_other, sg, sh).cuda()
    mask = (None if c["feat_mask"] is None
            else torch.from_numpy(c["feat_mask"]).cuda())
    return c, sg, sh, i_small, i_other, small, other, mask


def _scan(c, parent, small, small_is_left, mask, sg, sh):
    return backend.sibling_scan(parent, small, small_is_left, c["n_bins"],
                                c["l1"], c["l2"], c["min_data"],
                                c["min_hess"], c["nf_real"], mask, sg, sh)


def _check_records(name, rec, hist_ids, hists_q, mask, sg, sh):
    """rec (nh, nf_pad, 6) of the int64 histograms hists_q, which are the
    case's histograms hist_ids: the host arg-max names the oracle's split,
    and every record is split_scan's on the float histogram, bit for bit."""
    c = sc.cases()[name]
    o = sc.expected(name)
    nf_pad, nb = c["hists"].shape[1:3]
    assert rec.shape == (len(hist_ids), nf_pad, 6)
    assert rec.dtype == torch.float32
    rec = rec.cpu().numpy()
    inv = torch.tensor([1.0 / sg, 1.0 / sh, 1.0], dtype=torch.float64,
                       device="cuda")
    live = np.arange(nf_pad) < c["nf_real"]
    if c["feat_mask"] is not None:
        live &= c["feat_mask"]
    for row, (hi, hq) in enumerate(zip(hist_ids, hists_q)):
        histf = (hq.double() * inv).float()         # _to_float_hist's form
        assert np.array_equal(_bits(histf.cpu().numpy()),
                              _bits(c["hists"][hi]))
        # host arg-max, lowest feature on ties
        f = int(np.argmax(rec[row, :, 0]))
        bg, bf, bb = o["best"][hi]
        if bf is None:
            assert rec[row, f, 0] == -np.inf
        else:
            assert (f, int(rec[row, f, 2])) == (bf, bb), (name, row)
            assert rec[row, f, 1] == f
        whole = backend.split_scan(histf.unsqueeze(0), nb, c["l1"], c["l2"],
                                   c["min_data"], c["min_hess"], 0.0,
                                   c["nf_real"], mask).cpu().numpy()[0]
        if bf is not None:
            assert np.array_equal(_bits(whole), _bits(rec[row, f]))
        # per feature: every feature as a one-feature histogram of its own
        per_f = backend.split_scan(histf.unsqueeze(1), nb, c["l1"], c["l2"],
                                   c["min_data"], c["min_hess"], 0.0, 1,
                                   None).cpu().numpy()
        cols = [0, 2, 3, 4, 5]
        assert np.array_equal(_bits(rec[row][live][:, cols]),
                              _bits(per_f[live][:, cols]))
        assert np.array_equal(rec[row][live][:, 1],
                              np.arange(nf_pad, dtype=np.float32)[live])
        assert np.array_equal(_bits(rec[row][~live]),
                              _bits(np.tile(DEAD, ((~live).sum(), 1))))


@requires_gpu
@pytest.mark.parametrize("wide", [False, True], ids=["scale44", "scale60"])
@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_sibling_scan_subtracts_exactly_and_scans_like_split_scan(name, wide):
    c, sg, sh, i_small, i_other, small, other, mask = _sibling_inputs(
        name, wide)
    parent = small + other
    if wide:        # g cells of about 2^60, as under the grower's own scale
        assert 2 ** 58 <= int(parent[..., 0].abs().max()) < 2 ** 61
    parent0, small0 = parent.clone(), small.clone()
    for small_is_left in (True, False):
        rec, big = _scan(c, parent, small, small_is_left, mask, sg, sh)
        assert big.dtype == torch.int64 and big.shape == small.shape
        assert torch.equal(big, other)      # pad and masked cells included
        assert torch.equal(parent, parent0) and torch.equal(small, small0)
        ids, hq = (i_small, i_other), (small, big)
        if not small_is_left:
            ids, hq = ids[::-1], hq[::-1]
        _check_records(name, rec, ids, hq, mask, sg, sh)
    rec, big = _scan(c, None, small, True, mask, sg, sh)     # the root form
    assert big is None
    assert torch.equal(small, small0)
    _check_records(name, rec, (i_small,), (small,), mask, sg, sh)


# ----------------------------------------------------------- rejections
# Every call below stops at an argument check of the binding: none reaches a
# kernel launch.
def _good(nb=16, nf_pad=8):
    return torch.zeros(2, nf_pad, nb, 3, device="cuda")


@requires_gpu
def test_split_scan_rejects_bad_arguments():
    def call(h, nb, nf_real=8, mask=None):
        return backend.split_scan(h, nb, 0.0, 0.0, 1.0, 0.0, 0.0, nf_real,
                                  mask)

    assert call(_good(), 16).shape == (2, 6)                # the good call
    ok_mask = torch.ones(8, dtype=torch.bool, device="cuda")
    assert call(_good(), 16, 8, ok_mask).shape == (2, 6)
    for h, nb in ((_good(257), 257),                        # LDS holds 256
                  (_good(1), 1),
                  (_good(16), 15), (_good(16), 17), (_good(16), 255),
                  (_good()[0], 16),                         # 3-D
                  (_good().double(), 16),
                  (torch.zeros(2, 8, 16, 4, device="cuda"), 16)):
        with pytest.raises(RuntimeError):
            call(h, nb)
    with pytest.raises(RuntimeError):       # a CPU histogram, past backend
        backend._require_ext().split_scan(_good().cpu(), 16, 0.0, 0.0, 1.0,
                                          0.0, 0.0, 8, None)
    for nf_real in (0, -1, 9):
        with pytest.raises(RuntimeError):
            call(_good(), 16, nf_real)
    for mask in (torch.ones(8, dtype=torch.bool),                 # on the CPU
                 torch.ones(7, dtype=torch.bool, device="cuda"),  # too short
                 torch.ones(8, dtype=torch.uint8, device="cuda"),
                 torch.ones(16, dtype=torch.bool, device="cuda")[::2]):
        with pytest.raises(RuntimeError):
            call(_good(), 16, 8, mask)


@requires_gpu
def test_sibling_scan_rejects_bad_arguments():
    def small(nb=16, nf_pad=8, dtype=torch.int64):
        return torch.zeros(nf_pad, nb, 3, dtype=dtype, device="cuda")

    def call(parent, s, nb, nf_real=8, mask=None, sg=1.0, sh=1.0):
        return backend.sibling_scan(parent, s, True, nb, 0.0, 0.0, 1.0, 0.0,
                                    nf_real, mask, sg, sh)

    rec, big = call(small(), small(), 16)                   # the good call
    assert rec.shape == (2, 8, 6) and big.shape == (8, 16, 3)
    for s, nb in ((small(257), 257), (small(1), 1), (small(16), 15),
                  (small(16), 17), (small(dtype=torch.int32), 16),
                  (small().float(), 16), (small()[0], 16),
                  (torch.zeros(8, 16, 4, dtype=torch.int64, device="cuda"),
                   16),
                  (torch.zeros(8, 32, 3, dtype=torch.int64,
                               device="cuda")[:, ::2], 16)):
        with pytest.raises(RuntimeError):
            call(None, s, nb)
    with pytest.raises(RuntimeError):
        call(None, small().cpu(), 16)
    for parent in (small(16, 7), small(15), small().cpu(),
                   small(dtype=torch.int32)):
        with pytest.raises(RuntimeError):
            call(parent, small(), 16)
    for nf_real in (0, -1, 9):
        with pytest.raises(RuntimeError):
            call(None, small(), 16, nf_real)
    for mask in (torch.ones(8, dtype=torch.bool),
                 torch.ones(7, dtype=torch.bool, device="cuda"),
                 torch.ones(8, dtype=torch.uint8, device="cuda"),
                 torch.ones(16, dtype=torch.bool, device="cuda")[::2]):
        with pytest.raises(RuntimeError):
            call(None, small(), 16, 8, mask)
    for sg, sh in ((0.0, 1.0), (1.0, -2.0)):
        with pytest.raises(RuntimeError):
            call(None, small(), 16, 8, None, sg, sh)
