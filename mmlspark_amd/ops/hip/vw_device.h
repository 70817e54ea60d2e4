// Device helpers shared by the VW kernels (vw_kernels.hip and
// vw_interact_kernels.hip): the wave reduction, the loss derivative and the
// --invariant prediction-space move.
#pragma once
#include <hip/hip_runtime.h>

#define WAVE 64

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

// loss: 0=squared 1=logistic(label ±1) 2=hinge(label ±1)
__device__ __forceinline__ float dloss(int loss, float pred, float y) {
  switch (loss) {
    case 0: return pred - y;
    case 1: { // d/dp log(1+exp(-y p)) = -y * sigmoid(-y p)
      const float z = -y * pred;
      const float s = 1.0f / (1.0f + __expf(-z));
      return -y * s;
    }
    case 2: return (y * pred < 1.0f) ? -y : 0.0f;
  }
  return 0.0f;
}

// Importance-weight-invariant prediction-space move (VW --invariant,
// Karampatziakis & Langford): exact integral of dp/dh = -eta*dloss(p),
// never overshoots the label/margin for any importance weight h.
__device__ __forceinline__ float invariant_dp(int loss, float pred, float y,
                                              float h_eta) {
  switch (loss) {
    case 0:  // squared: p(h) = y + (p0-y) e^{-h eta}
      return (y - pred) * (-expm1f(-h_eta));
    case 1: {  // logistic: q=y*p obeys e^q + q = e^{q0}+q0+h_eta
      const float q0 = y * pred;
      // A = e^{q0} >= e^30: the linear term is below float resolution
      if (q0 > 30.0f) return y * (h_eta * __expf(-q0));
      // d = q-q0 >= 0 is the root of g(d) = A*expm1(d) + d - h_eta, convex
      // and increasing, so Newton started at or right of the root descends
      // onto it and never passes it.  Both h_eta (g = A*expm1) and
      // log1p(h_eta/A) (g = d) are right of it; the smaller is within a few
      // steps of it for every (q0, h_eta).  Where A underflows,
      // log1p(h_eta/A) = log(h_eta) - q0.
      const float start = q0 > -40.0f ? log1pf(h_eta / expf(q0))
                                      : logf(h_eta) - q0;
      float d = fminf(h_eta, fmaxf(start, 0.0f));
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        // A*e^d as e^{q0+d} (<= A + h_eta: no overflow) and A*expm1(d) as
        // that times (1 - e^{-d}): finite for every q0 and d
        const float E = expf(q0 + d);
        const float g = E * (-expm1f(-d)) + d - h_eta;
        d = fmaxf(d - g / (E + 1.0f), 0.0f);
      }
      return y * d;
    }
    case 2: {  // hinge: move to the margin, never past
      const float q0 = y * pred;
      return y * fminf(h_eta, fmaxf(1.0f - q0, 0.0f));
    }
  }
  return 0.0f;
}
