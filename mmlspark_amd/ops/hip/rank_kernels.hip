// Learning-to-rank kernels for gfx950: in-group ranks and lambdarank
// gradients for every query group of a training set in two launches whose
// count does not depend on the number of groups.
//
// Both kernels are thread-per-document, 256-thread blocks, grid ceil(n/256).
// A thread walks the documents of its own group, [offsets[g], offsets[g+1]).
// Neighbouring lanes share a group, so their partner loads coincide; a group
// costs O(m^2) whatever its size.  No atomics: each thread sums its own
// addends in increasing partner index, so results repeat from call to call.
//
// The group table comes from the host, which validates it once per fit
// (models/gbdt/ranking.py).  The kernels still clamp what they index with:
// a group id outside [0, G) or a range outside [0, n) yields zeros, never an
// out-of-bounds access.
#include <hip/hip_runtime.h>

// One 16-byte record per document: score, label, gain and the discount of
// the document's current rank.  lambdarank_grad_k does a single load per
// partner.
struct __align__(16) RankRec {
  float s, label, gain, disc;
};

__device__ __forceinline__ bool group_range(const long* __restrict__ offsets,
                                            const int* __restrict__ gid,
                                            long i, long n, int n_groups,
                                            int* g, long* b, long* e) {
  *g = gid[i];
  if (*g < 0 || *g >= n_groups) return false;
  *b = offsets[*g];
  *e = offsets[*g + 1];
  return *b >= 0 && *e <= n && *b <= *e;
}

// rank[i] = #{ j in group(i) : s_j > s_i || (s_j == s_i && j < i) }: the
// stable descending order.  A count, so it is in [0, m) whatever the scores
// are (NaN compares false both ways).
__global__ __launch_bounds__(256) void group_rank_k(
    const float* __restrict__ score, const long* __restrict__ offsets,
    const int* __restrict__ gid, const float* __restrict__ label,
    const float* __restrict__ gain, const float* __restrict__ disc_tbl,
    long n, int n_groups, long n_disc, int* __restrict__ rank,
    RankRec* __restrict__ rec) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float si = score[i];
  int g;
  long b, e;
  int r = 0;
  if (group_range(offsets, gid, i, n, n_groups, &g, &b, &e)) {
    for (long j = b; j < e; ++j) {
      const float sj = score[j];
      r += (sj > si) || (sj == si && j < i);
    }
  }
  rank[i] = r;
  RankRec out;
  out.s = si;
  out.label = label[i];
  out.gain = gain[i];
  out.disc = r < n_disc ? disc_tbl[r] : 0.0f;
  rec[i] = out;
}

// Lambdarank gradient and hessian of document i over every partner j of its
// group with a different label.  With hi the higher-labelled of the two and
// x = sigma * (s_hi - s_lo):
//   e = expf(-|x|), q = 1 / (1 + e), rho = x < 0 ? q : e * q   (= sigmoid(-x))
//   delta = |gain_i - gain_j| * |disc_i - disc_j| * inv_idcg[group]
//   g_i -/+= sigma * rho * delta          (- when i is hi)
//   h_i  += sigma^2 * (e * q * q) * delta (= rho * (1 - rho), never formed
//                                            as a difference)
// Nothing overflows for large |x|; expf and IEEE division, no fast math.
__global__ __launch_bounds__(256) void lambdarank_grad_k(
    const RankRec* __restrict__ rec, const long* __restrict__ offsets,
    const int* __restrict__ gid, const float* __restrict__ inv_idcg,
    float sigma, long n, int n_groups, float* __restrict__ grad,
    float* __restrict__ hess) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int g;
  long b, e;
  float ag = 0.0f, ah = 0.0f;
  if (group_range(offsets, gid, i, n, n_groups, &g, &b, &e)) {
    const RankRec ri = rec[i];
    const float inv = inv_idcg[g];
    const float sigma2 = sigma * sigma;
    for (long j = b; j < e; ++j) {
      const RankRec rj = rec[j];
      if (ri.label != rj.label) {
        const bool i_hi = ri.label > rj.label;
        const float x = sigma * (i_hi ? ri.s - rj.s : rj.s - ri.s);
        const float ex = expf(-fabsf(x));
        const float q = 1.0f / (1.0f + ex);
        const float eq = ex * q;
        const float rho = x < 0.0f ? q : eq;
        const float delta =
            fabsf(ri.gain - rj.gain) * fabsf(ri.disc - rj.disc) * inv;
        const float t = sigma * rho * delta;
        ag += i_hi ? -t : t;
        ah += sigma2 * (eq * q) * delta;
      }
    }
  }
  grad[i] = ag;
  hess[i] = ah;
}

extern "C" void launch_group_rank(const float* score, const long* offsets,
                                  const int* gid, const float* label,
                                  const float* gain, const float* disc_tbl,
                                  long n, int n_groups, long n_disc, int* rank,
                                  void* rec, hipStream_t stream) {
  if (n == 0) return;
  const long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(group_rank_k, dim3((unsigned)blocks), dim3(256), 0,
                     stream, score, offsets, gid, label, gain, disc_tbl, n,
                     n_groups, n_disc, rank, (RankRec*)rec);
}

extern "C" void launch_lambdarank_grad(const void* rec, const long* offsets,
                                       const int* gid, const float* inv_idcg,
                                       float sigma, long n, int n_groups,
                                       float* grad, float* hess,
                                       hipStream_t stream) {
  if (n == 0) return;
  const long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(lambdarank_grad_k, dim3((unsigned)blocks), dim3(256), 0,
                     stream, (const RankRec*)rec, offsets, gid, inv_idcg,
                     sigma, n, n_groups, grad, hess);
}
