"""GPU test for the range-mode arena histogram (`hist_pair_range`, the kernel
behind every child histogram of the native GBDT grower) against an exact
int64 oracle computed on the CPU with one `index_add_` per feature.

The sums are integers, so everything is compared for equality: the rows of
the real features, and the rows of the pad features of the last bin plane,
which the kernel must leave as it found them."""
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs ROCm GPU")

N_ARENA = 10_000
N_BINS = 255
CNT = 1 << 44  # the count bit that rides in the hessian word
# ranges (lo, m) across the 256-row tile and the 4 x 256 unrolled step
RANGES = [(0, 1), (0, 64), (37, 255), (37, 256), (37, 257), (0, 1024),
          (5, 1025), (0, 4097), (0, N_ARENA)]
CHUNKS = [0, 256, 1280]  # the launcher's policy, one tile, one step + a tile


def _arena(nf, seed):
    """Random arena on the CPU.  Every byte of every plane is a valid bin,
    pad bytes included, so a kernel that read a pad byte would show."""
    g = torch.Generator().manual_seed(seed)
    npairs = (nf + 7) // 8
    by = torch.randint(0, N_BINS, (npairs, N_ARENA, 8), generator=g,
                       dtype=torch.uint8)
    pair = by.view(torch.int64).squeeze(-1).contiguous()
    gq = torch.randint(-2**40, 2**40, (N_ARENA,), generator=g,
                       dtype=torch.int64)
    hq = torch.randint(0, 2**24, (N_ARENA,), generator=g, dtype=torch.int64)
    ghq = torch.stack([gq, hq | CNT], dim=1).contiguous()
    # (nf, N_ARENA) bin ids, feature-major, for the oracle
    bins = by.permute(0, 2, 1).reshape(npairs * 8, N_ARENA)[:nf].long()
    return pair, ghq, bins.contiguous(), gq, hq


class _Oracle:
    """Exact histogram of rows [a, a+k) — computed once per distinct range."""

    def __init__(self, nf, bins, gq, hq):
        self.nf, self.bins, self.gq, self.hq = nf, bins, gq, hq
        self.cache = {}

    def __call__(self, a, k):
        if (a, k) not in self.cache:
            npairs = (self.nf + 7) // 8
            out = torch.zeros(npairs * 8, N_BINS, 3, dtype=torch.int64)
            vals = torch.stack([self.gq[a:a + k], self.hq[a:a + k],
                                torch.ones(k, dtype=torch.int64)], dim=1)
            for f in range(self.nf):
                out[f].index_add_(0, self.bins[f, a:a + k], vals)
            self.cache[(a, k)] = out
        return self.cache[(a, k)]


@requires_gpu
@pytest.mark.parametrize("nf", [5, 12, 100])
def test_hist_pair_range_matches_int64_oracle(nf):
    """nf = 5 / 12 / 100 give 1 / 2 / 13 planes with 5 / 4 / 4 valid bytes in
    the last one.  side = 0 / 1 read the left / right part of the range as
    split by a device count of 0, m and an interior value.  The slab starts
    from a non-zero base, so the result proves `+=`."""
    from mmlspark_amd.ops import _hip_grower
    pair, ghq, bins, gq, hq = _arena(nf, seed=300 + nf)
    npairs = (nf + 7) // 8
    tail_bytes = nf - (npairs - 1) * 8
    assert tail_bytes == {5: 5, 12: 4, 100: 4}[nf]
    oracle = _Oracle(nf, bins, gq, hq)
    pair_d, ghq_d = pair.cuda(), ghq.cuda()
    g = torch.Generator().manual_seed(nf)
    base = torch.randint(1, 1000, (npairs * 8, N_BINS, 3), generator=g,
                         dtype=torch.int64)
    base_d = base.cuda()
    for lo, m in RANGES:
        sides = [(-1, None)]
        for nl in sorted({0, m // 3, m}):
            sides += [(0, nl), (1, nl)]
        for chunk in CHUNKS:
            for side, nl in sides:
                hist = base_d.clone()
                nl_dev = (None if nl is None else
                          torch.tensor([nl], dtype=torch.int32, device="cuda"))
                _hip_grower.hist_pair_range(pair_d, ghq_d, lo, m, hist,
                                            N_BINS, tail_bytes, nl_dev, side,
                                            chunk)
                if side < 0:
                    a, k = lo, m
                elif side == 0:
                    a, k = lo, nl
                else:
                    a, k = lo + nl, m - nl
                expect = base + oracle(a, k)
                got = hist.cpu()
                tag = (lo, m, chunk, side, nl)
                assert torch.equal(got[:nf], expect[:nf]), tag
                # pad features: nothing added
                assert torch.equal(got[nf:], base[nf:]), tag
    # the oracle itself saw every bin edge and a real spread of sums
    full = oracle(0, N_ARENA)
    assert int(full[:nf, :, 2].sum()) == nf * N_ARENA
    assert (full[:nf, 0, 2] > 0).all() and (full[:nf, N_BINS - 1, 2] > 0).all()


@requires_gpu
def test_hist_pair_range_rejects_bad_arguments():
    from mmlspark_amd.ops import _hip_grower
    pair, ghq, _, _, _ = _arena(12, seed=1)
    pair_d, ghq_d = pair.cuda(), ghq.cuda()
    hist = torch.zeros(16, N_BINS, 3, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="range out of bounds"):
        _hip_grower.hist_pair_range(pair_d, ghq_d, 1, N_ARENA, hist, N_BINS, 4)
    with pytest.raises(RuntimeError, match="hist"):
        _hip_grower.hist_pair_range(pair_d, ghq_d, 0, 10, hist[:8], N_BINS, 4)
    with pytest.raises(RuntimeError, match="nl_dev"):
        _hip_grower.hist_pair_range(pair_d, ghq_d, 0, 10, hist, N_BINS, 4,
                                    None, 0)
    assert int(hist.abs().sum()) == 0
