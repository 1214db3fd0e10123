// Temperature scaling of the K-member x T-pass ensemble (gfx950): include/mmu.h mmu_temperature_nll.
//
// The ensemble NLL under J candidate inverse-temperature vectors beta_j in R^K, in one read of the
// logit stack, by the row scheme of ensemble_rows.h with the waves sharing member k's T rows; the
// softmax is per candidate, so only the NJ dispatch is shared.  A row's max m is found once (max(beta z) =
// beta max z for every beta >= 0), and every candidate's term
//   exp(beta_jk (z_y - m)) / sum_c exp(beta_jk (z_c - m))
// comes from the row's registers.  Lane j of a wave holds beta_jk (fetched once per member), keeps
// candidate j's exp-sum of the row as the wave reduces it, forms the label's term once per row, and
// keeps candidate j's running sum (J <= 64: one VGPR each).  The waves' partial sums are folded in
// wave order by thread j, so a candidate's result does not depend on which other candidates share
// its launch.  No scratch.
#include "ensemble_rows.h"
#include "mmu_internal.h"

namespace mmu {

constexpr int TN_WAVES = 4;
constexpr int TN_THREADS = 64 * TN_WAVES;
// -ln 1e-12, the value a floored probability gets (a label outside [0, C), an underflowed p_y)
constexpr float TN_NLL_FLOOR = 27.6310211159285482f;

template <int NJ>
__global__ __launch_bounds__(TN_THREADS) void temperature_nll_kernel(
    const float* __restrict__ logits, int64_t ss, int64_t sk, int64_t st, const int64_t* __restrict__ y, int64_t K,
    int64_t T, int64_t C, const float* __restrict__ inv_temp, int J, float* __restrict__ nll) {
  __shared__ float part[TN_WAVES][64];
  const int64_t s = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t yy = y[s];
  const bool has_y = yy >= 0 && yy < C;  // compared, never indexed: outside [0, C) the label has p = 0
  const float invT = 1.0f / (float)T;
  float pacc = 0.f;  // thread j < J: sum_k p_k[y] under candidate j

  for (int64_t k = 0; k < K; ++k) {
    const float beta_l = lane < J ? inv_temp[(int64_t)lane * K + k] : 0.f;  // lane j: beta_jk
    float acc = 0.f;                                                        // lane j: this wave's sum over its rows
    for (int64_t t = wave; t < T; t += TN_WAVES) {
      const float* z = logits + s * ss + k * sk + t * st;
      // load_row written out: on the helper the NJ = 4 instantiation measured 3 % slower (C = 200)
      float d[NJ];
      float m = -__builtin_huge_valf();
#pragma unroll
      for (int i = 0; i < NJ; ++i) {
        const int c = lane + 64 * i;
        d[i] = c < C ? z[c] : -__builtin_huge_valf();
        m = fmaxf(m, d[i]);
      }
      m = wave_max(m);
      float dy = 0.f;
#pragma unroll
      for (int i = 0; i < NJ; ++i) {
        d[i] -= m;
        dy += has_y && (int64_t)(lane + 64 * i) == yy ? d[i] : 0.f;  // one owner lane, the others add 0
      }
      dy = wave_sum(dy);
      float se_l = 1.f;  // lane j: candidate j's exp-sum of this row
      for (int j = 0; j < J; ++j) {
        const float beta = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, beta_l), j));
        float se = 0.f;
#pragma unroll
        for (int i = 0; i < NJ; ++i) se += lane + 64 * i < C ? expf(beta * d[i]) : 0.f;
        se = wave_sum(se);
        se_l = lane == j ? se : se_l;
      }
      // the label's term once per row, by the lane that owns the candidate
      acc += has_y && lane < J ? expf(beta_l * dy) / se_l : 0.f;
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (tid < J) {
      float pk = part[0][tid];
#pragma unroll
      for (int w = 1; w < TN_WAVES; ++w) pk += part[w][tid];
      pacc += pk * invT;
    }
    __syncthreads();
  }
  if (tid < J) {
    const float p = pacc * (1.0f / (float)K);
    nll[s * J + tid] = p > 1e-12f ? -logf(p) : TN_NLL_FLOOR;
  }
}

// nll_sum[j] = sum_s nll[s, j] in f64: one wave per candidate, as ece_bins_det_kernel.  Lane l walks
// samples l, l + 64, ... in index order; the 64 lane sums are folded by a fixed butterfly.
__global__ __launch_bounds__(64) void temperature_nll_sum_kernel(const float* __restrict__ nll, int64_t S, int J,
                                                                 double* __restrict__ nll_sum) {
  const int j = blockIdx.x;
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < S; i += 64) a += (double)nll[i * J + j];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if (threadIdx.x == 0) nll_sum[j] = a;
}

void temperature_nll_launch(const float* logits, int64_t ss, int64_t sk, int64_t st, const int64_t* y, int64_t S,
                            int64_t K, int64_t T, int64_t C, const float* inv_temp, int64_t J, float* nll,
                            double* nll_sum, hipStream_t s) {
  dispatch_nj(C, [&](auto nj) {
    hipLaunchKernelGGL(temperature_nll_kernel<decltype(nj)::value>, dim3((unsigned)S), dim3(TN_THREADS), 0, s, logits,
                       ss, sk, st, y, K, T, C, inv_temp, (int)J, nll);
  });
  if (nll_sum)
    hipLaunchKernelGGL(temperature_nll_sum_kernel, dim3((unsigned)J), dim3(64), 0, s, nll, S, (int)J, nll_sum);
}

}  // namespace mmu
