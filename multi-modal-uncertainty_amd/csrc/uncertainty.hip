// Ensemble / MC-dropout uncertainty reduction (gfx950).
//
// North-star metrics.  Convention of the reference analysis code:
// softmax per member / pass, then the mean over members (notebooks/food101_robustness.py:25-36,
// notebooks/utils.py:22-23).  One 128-thread block per sample reduces R = K*T logit rows.
#include "ensemble_rows.h"
#include "mmu_internal.h"

namespace mmu {

__global__ __launch_bounds__(128) void uncertainty_kernel(const float* __restrict__ logits, const int64_t* __restrict__ y,
                                                          int64_t R, int64_t C, float* __restrict__ p_bar,
                                                          float* __restrict__ nll, float* __restrict__ conf,
                                                          float* __restrict__ correct) {
  __shared__ float red[2];
  __shared__ float acc[1024];
  const int64_t s = blockIdx.x;
  const int t = threadIdx.x;
  for (int c = t; c < C; c += 128) acc[c] = 0.f;
  for (int64_t r = 0; r < R; ++r) {
    const float* z = logits + (s * R + r) * C;
    float mx = -__builtin_huge_valf();
    for (int c = t; c < C; c += 128) mx = fmaxf(mx, z[c]);
    mx = wave_max(mx);
    if ((t & 63) == 0) red[t >> 6] = mx;
    __syncthreads();
    mx = fmaxf(red[0], red[1]);
    __syncthreads();
    float sm = 0.f;
    for (int c = t; c < C; c += 128) sm += __expf(z[c] - mx);
    sm = wave_sum(sm);
    if ((t & 63) == 0) red[t >> 6] = sm;
    __syncthreads();
    const float inv = 1.0f / (red[0] + red[1]);
    __syncthreads();
    for (int c = t; c < C; c += 128) acc[c] += __expf(z[c] - mx) * inv;
  }
  __syncthreads();
  const float invR = 1.0f / (float)R;
  float best = -1.f;
  int arg = 0;
  for (int c = t; c < C; c += 128) {
    const float pb = acc[c] * invR;
    p_bar[s * C + c] = pb;
    if (pb > best) { best = pb; arg = c; }
  }
  // argmax: first index of the maximum (ties -> lowest class, like torch/numpy argmax)
  for (int o = 32; o > 0; o >>= 1) {
    float ob = __shfl_xor(best, o, 64);
    int oa = __shfl_xor(arg, o, 64);
    if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
  }
  __shared__ float bb[2];
  __shared__ int ba[2];
  if ((t & 63) == 0) { bb[t >> 6] = best; ba[t >> 6] = arg; }
  __syncthreads();
  if (t == 0) {
    float b0 = bb[0];
    int a0 = ba[0];
    if (bb[1] > b0 || (bb[1] == b0 && ba[1] < a0)) { b0 = bb[1]; a0 = ba[1]; }
    const int64_t yy = y[s];
    nll[s] = -logf(fmaxf(acc[yy] * invR, 1e-12f));
    conf[s] = b0;
    correct[s] = a0 == yy ? 1.f : 0.f;
  }
}

// bin b holds conf in (b/n, (b+1)/n]; conf == 0 -> bin 0
__global__ void ece_bins_kernel(const float* __restrict__ conf, const float* __restrict__ correct, int64_t S,
                                int n_bins, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S) return;
  int b = (int)ceilf(conf[i] * n_bins) - 1;
  b = b < 0 ? 0 : (b >= n_bins ? n_bins - 1 : b);
  atomicAdd(out + 3 * b, 1.f);
  atomicAdd(out + 3 * b + 1, conf[i]);
  atomicAdd(out + 3 * b + 2, correct[i]);
}

void uncertainty_launch(const float* logits, const int64_t* y, int64_t S, int64_t R, int64_t C, float* p_bar,
                        float* nll, float* conf, float* correct, hipStream_t s) {
  hipLaunchKernelGGL(uncertainty_kernel, dim3((unsigned)S), dim3(128), 0, s, logits, y, R, C, p_bar, nll, conf, correct);
}

// Deterministic mode: one wave per bin, no atomics and no memset.  Lane l walks samples l, l + 64,
// ... in index order and keeps the bin's count / conf / correct sums of its own samples; the 64 lane
// sums are folded by the fixed butterfly of wave_sum, and lane 0 stores the bin's three figures.
__global__ __launch_bounds__(64) void ece_bins_det_kernel(const float* __restrict__ conf,
                                                          const float* __restrict__ correct, int64_t S, int n_bins,
                                                          float* __restrict__ out) {
  const int bin = blockIdx.x;
  float cnt = 0.f, sc = 0.f, sk = 0.f;
  for (int64_t i = threadIdx.x; i < S; i += 64) {
    const float c = conf[i];
    int b = (int)ceilf(c * n_bins) - 1;
    b = b < 0 ? 0 : (b >= n_bins ? n_bins - 1 : b);
    if (b == bin) {
      cnt += 1.f;
      sc += c;
      sk += correct[i];
    }
  }
  cnt = wave_sum(cnt);
  sc = wave_sum(sc);
  sk = wave_sum(sk);
  if (threadIdx.x == 0) {
    out[3 * bin] = cnt;
    out[3 * bin + 1] = sc;
    out[3 * bin + 2] = sk;
  }
}

void ece_bins_launch(const float* conf, const float* correct, int64_t S, int64_t n_bins, float* out, hipStream_t s) {
  if (deterministic()) {
    hipLaunchKernelGGL(ece_bins_det_kernel, dim3((unsigned)n_bins), dim3(64), 0, s, conf, correct, S, (int)n_bins, out);
    return;
  }
  (void)hipMemsetAsync(out, 0, sizeof(float) * 3 * n_bins, s);
  hipLaunchKernelGGL(ece_bins_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, s, conf, correct, S,
                     (int)n_bins, out);
}

// ------------------------------------------------------------------ entropy / mutual-information split
// The row scheme of ensemble_rows.h, the waves sharing member k's T rows.  Beside its share of the
// member's p_k a row gives its argmax vote and its entropy ln Z - sum e^(z-m) (z-m) / Z.  The waves'
// partial p_k meet in LDS and are folded in wave order by the thread that owns the class (tid,
// tid + 256, ...), which also keeps that class of p = mean_k p_k.  The per-row and per-member
// entropies are summed over rows / members in f64 (a handful of adds).
constexpr int UD_WAVES = 4;
constexpr int UD_THREADS = 64 * UD_WAVES;

// SCALED (mmu_uncertainty_decompose_scaled): member k's logits are multiplied by inv_temp[k] as they
// are loaded, and everything below sees beta_k z_kt; the unscaled instantiation never reads inv_temp.
template <int NJ, bool SCALED>
__global__ __launch_bounds__(UD_THREADS) void uncertainty_decompose_kernel(
    const float* __restrict__ logits, int64_t ss, int64_t sk, int64_t st, const int64_t* __restrict__ y, int64_t K,
    int64_t T, int64_t C, float* __restrict__ stats, float* __restrict__ p_bar, float* __restrict__ member_nll,
    const float* __restrict__ inv_temp) {
  constexpr int NI = NJ * 64 > UD_THREADS ? NJ * 64 / UD_THREADS : 1;  // classes per thread in the fold
  __shared__ float part[UD_WAVES][NJ * 64];
  __shared__ double red_d[UD_WAVES][4];
  __shared__ float red_f[UD_WAVES][2];
  __shared__ int red_i[UD_WAVES][2];
  const int64_t s = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t yy = y[s];
  const float invT = 1.0f / (float)T;
  float pacc[NI];   // sum_k p_k of the classes this thread folds
  int votes[NJ];    // this wave's row-argmax counts of the classes this lane owns
#pragma unroll
  for (int i = 0; i < NI; ++i) pacc[i] = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) votes[j] = 0;
  float hk = 0.f;     // this thread's share of sum_k H[p_k]
  double hrow = 0.0;  // this wave's sum of row entropies (wave-uniform)

  for (int64_t k = 0; k < K; ++k) {
    float acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = 0.f;
    float beta = 1.f;
    if constexpr (SCALED) beta = inv_temp[k];
    for (int64_t t = wave; t < T; t += UD_WAVES) {
      const float* z = logits + s * ss + k * sk + t * st;
      // load_row and softmax_accumulate written out, with the scale, the argmax, the entropy term sum e d
      // and the vote in their loops: on the helpers NJ = 16 takes 129 VGPRs for 117 and loses a wave
      float v[NJ];
      float best = -__builtin_huge_valf();
      int arg = lane;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int c = lane + 64 * j;
        if constexpr (SCALED) v[j] = c < C ? beta * z[c] : -__builtin_huge_valf();
        else v[j] = c < C ? z[c] : -__builtin_huge_valf();
        if (v[j] > best) { best = v[j]; arg = c; }
      }
      wave_argmax(best, arg);
      float se = 0.f, sd = 0.f;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const float d = v[j] - best;
        const float e = lane + 64 * j < C ? expf(d) : 0.f;
        v[j] = e;
        se += e;
        sd += e > 0.f ? e * d : 0.f;
        votes[j] += arg == lane + 64 * j ? 1 : 0;
      }
      se = wave_sum(se);
      sd = wave_sum(sd);
      hrow += (double)(logf(se) - sd / se);
      const float inv = 1.0f / se;
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[j] += v[j] * inv;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (lane + 64 * j < C) part[wave][lane + 64 * j] = acc[j];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int c = tid + UD_THREADS * i;
      if (c < C) {
        float pk = part[0][c];
#pragma unroll
        for (int w = 1; w < UD_WAVES; ++w) pk += part[w][c];
        pk *= invT;
        pacc[i] += pk;
        if (pk > 0.f) hk -= pk * logf(pk);
        if (member_nll && c == yy) member_nll[s * K + k] = -logf(fmaxf(pk, 1e-12f));
      }
    }
    __syncthreads();
  }

  // p, its entropy / Brier score / argmax, and the vote counts folded over the waves
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    if (lane + 64 * j < C) part[wave][lane + 64 * j] = __int_as_float(votes[j]);
  __syncthreads();
  const float invK = 1.0f / (float)K;
  float ent = 0.f, brier = 0.f, py = 0.f, best = -1.f;
  int arg = tid, vote = 0;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int c = tid + UD_THREADS * i;
    if (c < C) {
      const float p = pacc[i] * invK;
      p_bar[s * C + c] = p;
      if (p > 0.f) ent -= p * logf(p);
      const float d = p - (c == yy ? 1.f : 0.f);
      brier += d * d;
      if (c == yy) py = p;
      if (p > best) { best = p; arg = c; }
      int n = 0;
#pragma unroll
      for (int w = 0; w < UD_WAVES; ++w) n += __float_as_int(part[w][c]);
      vote = n > vote ? n : vote;
    }
  }
  ent = wave_sum(ent);
  hk = wave_sum(hk);
  brier = wave_sum(brier);
  py = wave_sum(py);  // one owner, the others hold 0
  wave_argmax(best, arg);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int ov = __shfl_xor(vote, o, 64);
    vote = ov > vote ? ov : vote;
  }
  if (lane == 0) {
    red_d[wave][0] = (double)ent;
    red_d[wave][1] = (double)hk;
    red_d[wave][2] = hrow;
    red_d[wave][3] = (double)brier;
    red_f[wave][0] = py;
    red_f[wave][1] = best;
    red_i[wave][0] = arg;
    red_i[wave][1] = vote;
  }
  __syncthreads();
  if (tid == 0) {
    double e = 0.0, h = 0.0, r = 0.0, b = 0.0;
    float p_y = 0.f, b0 = red_f[0][1];
    int a0 = red_i[0][0], v0 = 0;
    for (int w = 0; w < UD_WAVES; ++w) {
      e += red_d[w][0];
      h += red_d[w][1];
      r += red_d[w][2];
      b += red_d[w][3];
      p_y += red_f[w][0];
      if (red_f[w][1] > b0 || (red_f[w][1] == b0 && red_i[w][0] < a0)) { b0 = red_f[w][1]; a0 = red_i[w][0]; }
      v0 = red_i[w][1] > v0 ? red_i[w][1] : v0;
    }
    const double rows = (double)K * (double)T;
    const double hmem = h / (double)K, alea = r / rows;
    float* o = stats + s * MMU_UNC_NSTAT;
    o[MMU_UNC_TOTAL] = (float)e;
    o[MMU_UNC_ALEATORIC] = (float)alea;
    o[MMU_UNC_MI_MEMBERS] = (float)(e - hmem);
    o[MMU_UNC_MI_PASSES] = (float)(hmem - alea);
    o[MMU_UNC_BRIER] = (float)b;
    o[MMU_UNC_NLL] = -logf(fmaxf(p_y, 1e-12f));
    o[MMU_UNC_CONF] = b0;
    o[MMU_UNC_CORRECT] = a0 == yy ? 1.f : 0.f;
    o[MMU_UNC_VOTE_DISAGREEMENT] = (float)(1.0 - (double)v0 / rows);
  }
}

void uncertainty_decompose_launch(const float* logits, int64_t ss, int64_t sk, int64_t st, const int64_t* y, int64_t S,
                                  int64_t K, int64_t T, int64_t C, float* stats, float* p_bar, float* member_nll,
                                  const float* inv_temp, hipStream_t s) {
  dispatch_nj(C, [&](auto nj) {
    constexpr int NJ = decltype(nj)::value;
    if (inv_temp)
      hipLaunchKernelGGL((uncertainty_decompose_kernel<NJ, true>), dim3((unsigned)S), dim3(UD_THREADS), 0, s, logits,
                         ss, sk, st, y, K, T, C, stats, p_bar, member_nll, inv_temp);
    else
      hipLaunchKernelGGL((uncertainty_decompose_kernel<NJ, false>), dim3((unsigned)S), dim3(UD_THREADS), 0, s, logits,
                         ss, sk, st, y, K, T, C, stats, p_bar, member_nll, inv_temp);
  });
}

}  // namespace mmu
