// Modality-reliance summary of the robustness stack (gfx950): include/mmu.h mmu_robustness_summary.
//
// The formulas are those of the reference's analysis (notebooks/food101_robustness.py,
// notebooks/utils.py: label probability per variant, experimental shift against the mean control
// shift, argmax of the head-mean logits), restated; the Jensen-Shannon columns have no counterpart.
//
// The row scheme of ensemble_rows.h, but a wave reduces a whole variant (its K head rows): the
// row's softmax share of p_v and its share of the head-sum logits come from the row's registers.  Wave 0
// reduces variant 0 first and parks p_0 and H[p_0] in LDS; after one barrier wave w takes variants
// 1 + w, 5 + w, ... and forms each one's label probability, hit and divergence from p_0.  The
// per-variant triples meet in LDS, and threads 0 / 1 fold the image / text controls in index order
// (means, and the std as a two-pass sum, in f64).
#include "ensemble_rows.h"
#include "mmu_internal.h"

namespace mmu {

constexpr int RS_WAVES = 4;
constexpr int RS_THREADS = 64 * RS_WAVES;
constexpr int RS_MAXV = 1023;

// p_v = mean_k softmax(z[k, :]) in p[] (0 past C), zs[] = sum_k z[k, :] (-inf past C)
template <int NJ>
static __device__ __forceinline__ void rs_reduce_variant(const float* __restrict__ z, int64_t sk, int64_t K, int64_t C,
                                                         int lane, float (&p)[NJ], float (&zs)[NJ]) {
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    p[j] = 0.f;
    zs[j] = lane + 64 * j < C ? 0.f : -__builtin_huge_valf();
  }
  for (int64_t k = 0; k < K; ++k) {
    float v[NJ];
    const float mx = wave_max(load_row<NJ>(z + k * sk, C, lane, v));
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (lane + 64 * j < C) zs[j] += v[j];
    softmax_accumulate<NJ>(v, mx, C, lane, p);
  }
  const float invK = 1.0f / (float)K;
#pragma unroll
  for (int j = 0; j < NJ; ++j) p[j] *= invK;
}

// the variant's (p_label, hit, H[p_v]) from its registers; every lane ends with the same values
template <int NJ>
static __device__ __forceinline__ void rs_variant_stats(const float (&p)[NJ], const float (&zs)[NJ], int64_t K,
                                                        int64_t C, int64_t yy, int lane, float& pl, float& hit,
                                                        float& ent) {
  const float invK = 1.0f / (float)K;
  float best = -__builtin_huge_valf(), py = 0.f, h = 0.f;
  int arg = lane;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    if (c < C) {
      const float zm = zs[j] * invK;
      if (zm > best) { best = zm; arg = c; }
      if ((int64_t)c == yy) py = p[j];
      h -= xlogx(p[j]);
    }
  }
  wave_argmax(best, arg);
  pl = wave_sum(py);  // one owner, the others hold 0
  ent = wave_sum(h);
  hit = (int64_t)arg == yy ? 1.f : 0.f;
}

template <int NJ>
__global__ __launch_bounds__(RS_THREADS) void robustness_summary_kernel(
    const float* __restrict__ logits, int64_t ss, int64_t sv, int64_t sk, const int64_t* __restrict__ y, int64_t V,
    int64_t K, int64_t C, float* __restrict__ stats, float* __restrict__ per_variant) {
  __shared__ float p0[NJ * 64];
  __shared__ float h0;
  __shared__ float t_pl[RS_MAXV], t_js[RS_MAXV], t_hit[RS_MAXV];
  const int64_t s = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t yy = y[s];
  const float* zs0 = logits + s * ss;
  float p[NJ], zs[NJ];

  if (wave == 0) {
    rs_reduce_variant<NJ>(zs0, sk, K, C, lane, p, zs);
    float pl, hit, ent;
    rs_variant_stats<NJ>(p, zs, K, C, yy, lane, pl, hit, ent);
#pragma unroll
    for (int j = 0; j < NJ; ++j) p0[lane + 64 * j] = p[j];
    if (lane == 0) {
      h0 = ent;
      t_pl[0] = pl;
      t_js[0] = 0.f;  // the divergence of p_0 from itself
      t_hit[0] = hit;
    }
  }
  __syncthreads();
  const float ent0 = h0;
  for (int64_t v = 1 + wave; v < V; v += RS_WAVES) {
    rs_reduce_variant<NJ>(zs0 + v * sv, sk, K, C, lane, p, zs);
    float pl, hit, ent;
    rs_variant_stats<NJ>(p, zs, K, C, yy, lane, pl, hit, ent);
    float hm = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (lane + 64 * j < C) hm -= xlogx(0.5f * (p[j] + p0[lane + 64 * j]));
    hm = wave_sum(hm);
    if (lane == 0) {
      t_pl[v] = pl;
      t_js[v] = js_from_entropies(hm, ent, ent0);
      t_hit[v] = hit;
    }
  }
  __syncthreads();

  if (per_variant) {
    float* o = per_variant + s * 3 * V;
    for (int64_t v = tid; v < V; v += RS_THREADS) {
      o[v] = t_pl[v];
      o[V + v] = t_js[v];
      o[2 * V + v] = t_hit[v];
    }
  }
  if (tid < 2) {  // thread 0: the image columns, thread 1: the text columns
    const int64_t n = (V - 3) / 2, first = 3 + tid * n;
    const double pf = (double)t_pl[0];
    double dsum = 0.0, jsum = 0.0, hsum = 0.0;
    for (int64_t i = 0; i < n; ++i) {
      dsum += (double)t_pl[first + i] - pf;
      jsum += (double)t_js[first + i];
      hsum += (double)t_hit[first + i];
    }
    const double dmean = dsum / (double)n;
    double var = 0.0;
    for (int64_t i = 0; i < n; ++i) {
      const double d = ((double)t_pl[first + i] - pf) - dmean;
      var += d * d;
    }
    float* o = stats + s * MMU_ROB_NSTAT;
    const int m = 1 + tid;  // the modality's own variant
    o[tid ? MMU_ROB_DP_TEXT : MMU_ROB_DP_IMAGE] = (float)((double)t_pl[m] - pf);
    o[tid ? MMU_ROB_DP_TEXT_CONTROL : MMU_ROB_DP_IMAGE_CONTROL] = (float)dmean;
    o[tid ? MMU_ROB_SD_TEXT_CONTROL : MMU_ROB_SD_IMAGE_CONTROL] = (float)sqrt(var / (double)n);
    o[tid ? MMU_ROB_JS_TEXT : MMU_ROB_JS_IMAGE] = t_js[m];
    o[tid ? MMU_ROB_JS_TEXT_CONTROL : MMU_ROB_JS_IMAGE_CONTROL] = (float)(jsum / (double)n);
    o[tid ? MMU_ROB_HIT_TEXT : MMU_ROB_HIT_IMAGE] = t_hit[m];
    o[tid ? MMU_ROB_ACC_TEXT_CONTROL : MMU_ROB_ACC_IMAGE_CONTROL] = (float)(hsum / (double)n);
    if (tid == 0) {
      o[MMU_ROB_P_FULL] = t_pl[0];
      o[MMU_ROB_HIT_FULL] = t_hit[0];
    }
  }
}

void robustness_summary_launch(const float* logits, int64_t ss, int64_t sv, int64_t sk, const int64_t* y, int64_t S,
                               int64_t V, int64_t K, int64_t C, float* stats, float* per_variant, hipStream_t s) {
  dispatch_nj(C, [&](auto nj) {
    hipLaunchKernelGGL(robustness_summary_kernel<decltype(nj)::value>, dim3((unsigned)S), dim3(RS_THREADS), 0, s,
                       logits, ss, sv, sk, y, V, K, C, stats, per_variant);
  });
}

}  // namespace mmu
