// Ensemble diversity, per sample and per pair of members (gfx950): include/mmu.h mmu_ensemble_diversity.
//
// The analysis is the reference's "Prediction Diversity Analysis" (notebooks/analysis_round_1.py:68-113:
// mute the true class, keep each sub-network's top probabilities, Kendall tau between two of them),
// restated per sample; the Jensen-Shannon and disagreement columns have no counterpart.
//
// One 4-wave block per sample; LDS holds p_k = mean_t softmax(z[s, k, t, :]) of all K members
// (K rows of C rounded up to 64 floats, dynamic) and three K-entry tables.
//   Phase 1, the p_k, by the row scheme of ensemble_rows.h with the waves sharing member k's T rows.
//     The waves' shares are added into the member's LDS row one wave after the other (wave 0 stores,
//     wave 1 adds, ...; the last one scales by 1 / T): the sum and its order are those of the
//     decomposition's p_k.
//   Phase 2, per member (member k to wave k % 4): H[p_k], the argmax (ties to the lowest class) and
//     the truncation threshold, the m-th largest p_k[c] counted with multiplicity, by m rounds of a wave
//     argmax that each retire one class.
//   Phase 3, per pair (pair q to wave q % 4): the divergence from the entropies by a wave sum, and the
//     four Kendall counts by a sweep over the class pairs a < b: a lane keeps the truncated values of
//     its classes a of both members in registers, b walks the classes (an LDS broadcast), and only the
//     64-class groups that hold some a < b are visited.  The truncated vector is never stored:
//     x[c] = p[c] where p[c] >= thr and c is not the muted class, else 0.
// No scratch, and the counts are integers.
#include "ensemble_rows.h"
#include "mmu_internal.h"

namespace mmu {

constexpr int DV_WAVES = 4;
constexpr int DV_THREADS = 64 * DV_WAVES;
constexpr int DV_MAXK = 16;

// the truncated, muted value of class c
static __device__ __forceinline__ float dv_keep(float p, float thr, int c, int muted) {
  return p >= thr && c != muted ? p : 0.f;
}

template <int NJ>
__global__ __launch_bounds__(DV_THREADS) void ensemble_diversity_kernel(
    const float* __restrict__ logits, int64_t ss, int64_t sk, int64_t st, const int64_t* __restrict__ y, int K,
    int64_t T, int C, int top, int mute_true, float* __restrict__ pair, int32_t* __restrict__ counts,
    int32_t* __restrict__ member_arg) {
  extern __shared__ __attribute__((aligned(16))) char dv_smem[];
  const int CP = (C + 63) & ~63;  // a member's row
  float* const prob = reinterpret_cast<float*>(dv_smem);  // [K][CP]
  float* const t_thr = prob + (int64_t)K * CP;            // [DV_MAXK]
  float* const t_ent = t_thr + DV_MAXK;                   // [DV_MAXK]
  int* const t_arg = reinterpret_cast<int*>(t_ent + DV_MAXK);  // [DV_MAXK]
  const int64_t s = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t yy = y[s];
  // compared, never indexed: outside [0, C) no class is muted
  const int muted = mute_true && yy >= 0 && yy < C ? (int)yy : -1;

  // ---- phase 1: p_k into LDS
  const float invT = 1.0f / (float)T;
  const int nw = T < DV_WAVES ? (int)T : DV_WAVES;  // the waves that hold rows
  for (int k = 0; k < K; ++k) {
    float acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = 0.f;
    for (int64_t t = wave; t < T; t += DV_WAVES) {
      const float* z = logits + s * ss + k * sk + t * st;
      float v[NJ];
      const float mx = wave_max(load_row<NJ>(z, C, lane, v));
      softmax_accumulate<NJ>(v, mx, C, lane, acc);
    }
    float* pk = prob + k * CP;
    for (int w = 0; w < nw; ++w) {
      if (wave == w) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int c = lane + 64 * j;
          if (c < C) {
            float v = w ? pk[c] + acc[j] : acc[j];
            if (w == nw - 1) v *= invT;
            pk[c] = v;
          }
        }
      }
      __syncthreads();
    }
  }

  // ---- phase 2: per member, its entropy, argmax and threshold
  const int m = top < C ? top : C;  // 0: no truncation
  for (int k = wave; k < K; k += DV_WAVES) {
    const float* pk = prob + k * CP;
    float v[NJ];
    float h = 0.f, best = -2.f;
    int arg = lane;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = lane + 64 * j;
      v[j] = c < C ? pk[c] : -1.f;  // below every probability: never the maximum
      if (c < C) h -= xlogx(v[j]);
      if (v[j] > best) { best = v[j]; arg = c; }
    }
    h = wave_sum(h);
    wave_argmax(best, arg);
    const int amax = arg;
    float thr = 0.f;  // every class is kept
    unsigned gone = 0;  // bit j: class lane + 64 j has been counted
    for (int r = 0; r < m; ++r) {
      best = -2.f;
      arg = lane;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const float cand = (gone >> j) & 1u ? -1.f : v[j];
        if (cand > best) { best = cand; arg = lane + 64 * j; }
      }
      wave_argmax(best, arg);
      thr = best;
      if ((arg & 63) == lane) gone |= 1u << (arg >> 6);
    }
    if (lane == 0) {
      t_thr[k] = thr;
      t_ent[k] = h;
      t_arg[k] = amax;
      member_arg[s * K + k] = amax;
    }
  }
  __syncthreads();

  // ---- phase 3: per pair
  const int P = K * (K - 1) / 2;
  const int64_t n0 = (int64_t)C * (C - 1) / 2;
  for (int q = wave; q < P; q += DV_WAVES) {
    int i = 0, rem = q;  // itertools.combinations order
    while (rem >= K - 1 - i) { rem -= K - 1 - i; ++i; }
    const int jm = i + 1 + rem;
    const float* pi = prob + i * CP;
    const float* pj = prob + jm * CP;
    const float thr_i = t_thr[i], thr_j = t_thr[jm];
    float xi[NJ], xj[NJ];
    float hm = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = lane + 64 * j;
      const float a = c < C ? pi[c] : 0.f, b = c < C ? pj[c] : 0.f;
      hm -= xlogx(0.5f * (a + b));
      xi[j] = dv_keep(a, thr_i, c, muted);
      xj[j] = dv_keep(b, thr_j, c, muted);
    }
    hm = wave_sum(hm);
    int conc = 0, disc = 0, tx = 0, ty = 0;
    for (int b = 1; b < C; ++b) {
      const float bi = dv_keep(pi[b], thr_i, b, muted), bj = dv_keep(pj[b], thr_j, b, muted);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (64 * j < b) {  // wave-uniform: the group holds a class below b
          const bool in = lane + 64 * j < b;
          const int sx = (xi[j] > bi) - (xi[j] < bi), sy = (xj[j] > bj) - (xj[j] < bj);
          const int pr = sx * sy;
          conc += in && pr > 0;
          disc += in && pr < 0;
          tx += in && sx == 0;
          ty += in && sy == 0;
        }
      }
    }
    // (kept per lane: forming the four counts from lane masks and scalar population counts was
    // measured slower at C = 1024, 22.4 ms against 15.1 ms for S = 5000, K = 5, and no faster at C = 101)
    conc = wave_sum_int(conc);
    disc = wave_sum_int(disc);
    tx = wave_sum_int(tx);
    ty = wave_sum_int(ty);
    if (lane == 0) {
      const int64_t row = s * P + q;
      float* o = pair + row * MMU_DIV_NPAIR;
      o[MMU_DIV_JS] = js_from_entropies(hm, t_ent[i], t_ent[jm]);
      o[MMU_DIV_DISAGREE] = t_arg[i] != t_arg[jm] ? 1.f : 0.f;
      const int64_t dx = n0 - tx, dy = n0 - ty;
      o[MMU_DIV_TAU] = dx > 0 && dy > 0 ? (float)((double)(conc - disc) / sqrt((double)(dx * dy)))
                                         : __builtin_nanf("");
      if (counts) {
        int32_t* n = counts + row * 4;
        n[0] = conc;
        n[1] = disc;
        n[2] = tx;
        n[3] = ty;
      }
    }
  }
}

int64_t ensemble_diversity_lds_bytes(int64_t K, int64_t C) {
  return (int64_t)sizeof(float) * (K * ((C + 63) / 64 * 64) + 3 * DV_MAXK);
}

// -> hipSuccess, or why the LDS request of a launch above 64 KiB was turned down (nothing is launched then)
hipError_t ensemble_diversity_launch(const float* logits, int64_t ss, int64_t sk, int64_t st, const int64_t* y,
                                     int64_t S, int64_t K, int64_t T, int64_t C, int64_t top, int mute_true,
                                     float* pair, int32_t* counts, int32_t* member_arg, hipStream_t s) {
  const int64_t lds = ensemble_diversity_lds_bytes(K, C);
  return dispatch_nj(C, [&](auto nj) {
    constexpr int NJ = decltype(nj)::value;
    if (lds > 65536) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ensemble_diversity_kernel<NJ>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(ensemble_diversity_kernel<NJ>, dim3((unsigned)S), dim3(DV_THREADS), (size_t)lds, s, logits, ss,
                       sk, st, y, (int)K, T, (int)C, (int)top, mute_true, pair, counts, member_arg);
    return hipSuccess;
  });
}

}  // namespace mmu
