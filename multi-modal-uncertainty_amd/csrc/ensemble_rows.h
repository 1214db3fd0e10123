// Class rows of the ensemble's logit stack, shared by the per-sample statistics kernels
// (uncertainty.hip, calibration.hip, robustness.hip, diversity.hip; gfx950).
//
// One 4-wave block per sample.  A lane owns classes lane, lane + 64, ..., NJ per lane
// (NJ * 64 >= C, NJ <= 16) in registers: a logit row is loaded once, and its max, its softmax and
// whatever else a kernel takes from it come from those registers.  Where the rows of one member are
// averaged, the waves share its T rows (wave w takes t = w, w + 4, ...) and their partial sums meet
// in LDS.  No atomics: every sum has one fixed order, so a result depends on the inputs and the shape
// alone (the same launch in both modes of deterministic()).
#pragma once
#include <type_traits>
#include "mmu_common.h"

namespace mmu {

// argmax butterfly: ties go to the lowest class; every lane ends with the same pair
static __device__ __forceinline__ void wave_argmax(float& best, int& arg) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oa = __shfl_xor(arg, o, 64);
    if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
  }
}

static __device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

static __device__ __forceinline__ float xlogx(float p) { return p > 0.f ? p * logf(p) : 0.f; }

// v[j] = row[lane + 64 j], -inf past C -> the lane's max (wave_max of it is the row's)
template <int NJ, typename Int>
static __device__ __forceinline__ float load_row(const float* row, Int C, int lane, float (&v)[NJ]) {
  float mx = -__builtin_huge_valf();
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    v[j] = c < C ? row[c] : -__builtin_huge_valf();
    mx = fmaxf(mx, v[j]);
  }
  return mx;
}

// v[] becomes exp(v - mx) (0 past C), mx the row's max; acc[] += the row's softmax
template <int NJ, typename Int>
static __device__ __forceinline__ void softmax_accumulate(float (&v)[NJ], float mx, Int C, int lane,
                                                          float (&acc)[NJ]) {
  float se = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    v[j] = lane + 64 * j < C ? expf(v[j] - mx) : 0.f;
    se += v[j];
  }
  se = wave_sum(se);
  const float inv = 1.0f / se;
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] += v[j] * inv;
}

// Jensen-Shannon divergence of a and b from the entropies H[(a + b) / 2], H[a], H[b], closed in f64
static __device__ __forceinline__ float js_from_entropies(float hm, float ha, float hb) {
  return (float)((double)hm - 0.5 * ((double)ha + (double)hb));
}

// f(std::integral_constant<int, NJ>{}) with the smallest NJ in {1, 2, 4, 8, 16} that holds C <= 1024 classes
template <typename F>
static inline auto dispatch_nj(int64_t C, F&& f) {
  if (C <= 64) return f(std::integral_constant<int, 1>{});
  if (C <= 128) return f(std::integral_constant<int, 2>{});
  if (C <= 256) return f(std::integral_constant<int, 4>{});
  if (C <= 512) return f(std::integral_constant<int, 8>{});
  return f(std::integral_constant<int, 16>{});
}

}  // namespace mmu
