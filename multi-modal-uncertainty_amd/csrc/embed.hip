// Modality-token embedding + text gather + concat / control gather (gfx950).
//
// One pass builds the encoder input rows the reference assembles from
//   ImageBertEmbeddings   src/mmbt.py:58-83   ([CLS] | Linear(img) | [SEP], pos 0..N+1, type 0, LN)
//   BertEmbeddings        src/mmbt.py:121     (word[id] + pos[t] + type[seg], LN)
//   torch.cat             src/mmbt.py:122     (img tokens then text)
//   encoder_input[:, idx] src/mmbt.py:229     (forward_control gather, one index set per call)
// and the additive key mask (src/mmbt.py:101-112,203-216) for every output row, so
// the [B, L, H] activation (H = 768 or 1024) is written exactly once, already in its final order.
// Also: AdaptiveAvgPool2d((N,1)) of the ResNet map (src/mmbt.py:30,42-44) and the
// embedding backward (LN backward + word-row atomics + batch reductions).
#include "mmu_common.h"
#include "mmu_internal.h"

namespace mmu {


// Every row kernel here is templated on NV = H / 256 (3: bert-base, 4: bert-large), as layernorm.hip
// is: a wave holds a row as float[NV][4], lane l the columns 256 i + 4 l .. + 3.
template <int NV>
static __device__ __forceinline__ void add_row(float (&acc)[NV][4], const float* __restrict__ src, int l) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    float4 a = *(const float4*)(src + 256 * i + 4 * l);
    acc[i][0] += a.x; acc[i][1] += a.y; acc[i][2] += a.z; acc[i][3] += a.w;
  }
}

// pre-LN embedding sum of source position s for batch row b (H == 256 NV)
template <int NV>
static __device__ __forceinline__ void embed_sum(float (&e)[NV][4], const EmbedParams& p, int64_t b, int64_t s,
                                                 int l, float& km) {
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) e[i][k] = 0.f;
  const int64_t H = 256 * NV, nimg = p.n_img;
  km = 0.f;
  if (s <= nimg + 1) {
    if (s == 0) add_row(e, p.word + p.cls_id * H, l);
    else if (s == nimg + 1) add_row(e, p.word + p.sep_id * H, l);
    else add_row(e, p.proj + (b * nimg + (s - 1)) * H, l);
    add_row(e, p.pos + s * H, l);
    add_row(e, p.type, l);
  } else {
    const int64_t t = s - nimg - 2;
    const int64_t id = p.ids[b * p.T + t], sg = p.seg[b * p.T + t];
    add_row(e, p.word + id * H, l);
    add_row(e, p.pos + t * H, l);
    add_row(e, p.type + sg * H, l);
    if (p.txt_mask && p.txt_mask[b * p.T + t] == 0) km = -10000.0f;
  }
}

template <int NV>
__global__ __launch_bounds__(256) void embed_fwd_kernel(EmbedParams p) {
  constexpr int64_t H = 256 * NV;
  const int l = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t total = p.V * p.B * p.Lout;
  if (row >= total) return;
  const int64_t j = row % p.Lout, vb = row / p.Lout, b = vb % p.B, v = vb / p.B;
  const int64_t s = p.idx ? p.idx[v * p.Lout + j] : j;
  float e[NV][4], km;
  embed_sum<NV>(e, p, b, s, l, km);
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) sum += e[i][k];
  const float mu = wave_sum(sum) / (float)H;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) { float d = e[i][k] - mu; q += d * d; }
  const float rs = rsqrtf(wave_sum(q) / (float)H + p.eps);
  // dropout: ImageBertEmbeddings.dropout (p = args.dropout) on the image-segment rows,
  // BertEmbeddings.dropout (0.1) on text rows; element counter row*H + col (the
  // stream the GEMM and LayerNorm dropouts index the same way)
  const float dp = s <= p.n_img + 1 ? p.drop_img : p.drop_txt;
  const uint32_t thr = (uint32_t)(dp * 65536.0f + 0.5f);
  const float dsc = dp > 0.f ? 1.0f / (1.0f - dp) : 1.0f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = 256 * i + 4 * l;
    float4 w = *(const float4*)(p.ln_w + c), bb = *(const float4*)(p.ln_b + c);
    float y[4] = {(e[i][0] - mu) * rs * w.x + bb.x, (e[i][1] - mu) * rs * w.y + bb.y,
                  (e[i][2] - mu) * rs * w.z + bb.z, (e[i][3] - mu) * rs * w.w + bb.w};
    if (thr) {
      const uint32_t keep = mmu_keep4(mmu_eff_seed(p.seed, p.seed_off), (uint64_t)(row * H + c) >> 2, thr);
#pragma unroll
      for (int k = 0; k < 4; ++k) y[k] = ((keep >> k) & 1) ? y[k] * dsc : 0.f;
    }
    *(bf16x4*)(p.X + row * H + c) = bf16x4{f2bf(y[0]), f2bf(y[1]), f2bf(y[2]), f2bf(y[3])};
    if (p.X32) *(float4*)(p.X32 + row * H + c) = make_float4(y[0], y[1], y[2], y[3]);  // the f32 hidden stream
  }
  if (l == 0) {
    p.keymask[row] = km;
    if (p.mean) { p.mean[row] = mu; p.rstd[row] = rs; }
  }
}

void embed_fwd_launch(const EmbedParams& p, hipStream_t s) {
  const int64_t total = p.V * p.B * p.Lout;
  const dim3 grid((unsigned)((total + 3) / 4));
  if (p.H == 1024) hipLaunchKernelGGL(embed_fwd_kernel<4>, grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL(embed_fwd_kernel<3>, grid, dim3(256), 0, s, p);
}

// ---------------------------------------------------------------- backward
// One pass over the rows, position-major: a block = 4 consecutive source positions (one per wave)
// x EBW_B samples, so each wave sums its position's gradient over its samples in registers.  Per
// row: LN backward (dropout of the forward regenerated), the word-row scatter for text rows (f32
// atomics, 256 contiguous bytes per instruction), the image rows' dproj.  Per wave: its position
// sum into the position row / [CLS] / [SEP] word rows (f32 atomics, ceil(B / EBW_B) adds per
// address).  Per block: partial rows of dgamma, dbeta and the two token-type rows, folded by
// colsum_reduce.  (Round 6: the batch sums used to go through an f32 [B, S, H] copy of the row
// gradients and a second kernel walking it column-wise: 0.69 ms at B = 256 for 0.4 GB.)
constexpr int EBW_B = 16;  // samples per block
// DET (deterministic mode): no atomics.  A text row's dx goes to the scratch dxs [B * T, H] and
// the wave's position sum to postab [ceil(B / EBW_B), S, H], both behind the partial rows in q.ws
// (16 B per lane, whole lines); embed_bwd_launch sums them in a fixed order afterwards.
// LDS: the four kinds of partial rows are folded two at a time through red[2][4][H], so the block
// holds 12 H floats with xch instead of 20 H: 36,864 B at H = 768 (61,440 B before), 49,152 B at
// H = 1024, where the one-shot layout (81,920 B) would pass the 64 KiB static limit.  The sums and
// their order are the one-shot layout's.
// Compiler resource usage (-Rpass-analysis=kernel-resource-usage, gfx950), NV = 4:
//   atomics (DET = false): 49,152 B LDS, 193 VGPRs, 0 B scratch, 2 waves / SIMD;
//   DET = true (xch unused): 32,768 B LDS, 186 VGPRs, 0 B scratch, 2 waves / SIMD.
// NV = 3: 36,864 B / 161 VGPRs and 24,576 B / 151 VGPRs, 0 B scratch, 3 waves / SIMD.
// embed_fwd_kernel<4>: no LDS, 60 VGPRs, 0 B scratch.
template <int NV, bool DET>
__global__ __launch_bounds__(256) void embed_bwd_rows_kernel(EmbedBwdParams q, EmbedParams p) {
  constexpr int64_t H = 256 * NV;
  __shared__ float red[2][4][H];                            // per wave: aw, ab; then type-0, type-1
  __shared__ __attribute__((aligned(16))) float xch[4][H];  // per wave: a text row's dx, re-read lane-contiguous
  const int l = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t S = q.n_img + 2 + q.T;
  const int64_t nblk = (int64_t)gridDim.x * gridDim.y;
  const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  float* part = q.ws;
  float* dxs = q.ws + 4 * nblk * H;
  float* postab = dxs + q.B * q.T * H;
  const int64_t s = (int64_t)blockIdx.x * 4 + wv;
  const int64_t b0 = (int64_t)blockIdx.y * EBW_B;
  const bool live = s < S;
  const bool text = s >= q.n_img + 2, img = s >= 1 && s <= q.n_img;
  const float dp = s <= q.n_img + 1 ? q.drop_img : q.drop_txt;
  const uint32_t thr = (uint32_t)(dp * 65536.0f + 0.5f);
  const float dsc = dp > 0.f ? 1.0f / (1.0f - dp) : 1.0f;
  float aw[NV][4], ab[NV][4], w[NV][4], tot[NV][4], t1[NV][4];
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      aw[i][k] = ab[i][k] = tot[i][k] = t1[i][k] = 0.f;
      w[i][k] = q.ln_w[256 * i + 4 * l + k];
    }
  for (int64_t b = b0; live && b < b0 + EBW_B && b < q.B; ++b) {
    const int64_t row = b * S + s;
    float e[NV][4], km;
    embed_sum<NV>(e, p, b, s, l, km);
    const float mu = q.mean[row], rs = q.rstd[row];
    float g[NV][4], xh[NV][4], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      bf16x4 d = *(const bf16x4*)(q.dX + row * H + 256 * i + 4 * l);
      const uint32_t keep = thr ? mmu_keep4(mmu_eff_seed(q.seed, q.seed_off), (uint64_t)(row * H + 256 * i + 4 * l) >> 2, thr) : 0xFu;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float dy = ((keep >> k) & 1) ? bf2f(d[k]) * dsc : 0.f;
        xh[i][k] = (e[i][k] - mu) * rs;
        g[i][k] = dy * w[i][k];
        s1 += g[i][k];
        s2 += g[i][k] * xh[i][k];
        aw[i][k] += dy * xh[i][k];
        ab[i][k] += dy;
      }
    }
    s1 = wave_sum(s1) / (float)H;
    s2 = wave_sum(s2) / (float)H;
    const bool seg1 = text && q.seg[b * q.T + (s - q.n_img - 2)] != 0;
    float* wrow = text ? q.d_word + q.ids[b * q.T + (s - q.n_img - 2)] * H : nullptr;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = 256 * i + 4 * l;
      float dx[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        dx[k] = rs * (g[i][k] - s1 - xh[i][k] * s2);
        tot[i][k] += dx[k];
        if (seg1) t1[i][k] += dx[k];
      }
      if (text) {
        if (DET)
          *(float4*)(dxs + (b * q.T + (s - q.n_img - 2)) * H + c) = make_float4(dx[0], dx[1], dx[2], dx[3]);
        else
          *(float4*)(&xch[wv][c]) = make_float4(dx[0], dx[1], dx[2], dx[3]);
      } else if (img) {
        *(float4*)(q.d_proj + (b * q.n_img + (s - 1)) * H + c) = make_float4(dx[0], dx[1], dx[2], dx[3]);
      }
    }
    if (text && !DET) {  // word-row scatter: every atomic instruction adds 256 contiguous bytes (lane l ->
                 // column 64 j + l); 16-B-strided lanes ran the memory-side atomics at a fraction
                 // of their rate.  The row sits in this wave's own LDS slice: in-order LDS, no barrier.
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int j = 0; j < 4 * NV; ++j) atomicAdd(wrow + 64 * j + l, xch[wv][64 * j + l]);
      __builtin_amdgcn_wave_barrier();
    }
  }
  if (live && DET) {  // this position's sum over the block's samples: its row of the block's table slab
#pragma unroll
    for (int i = 0; i < NV; ++i)
      *(float4*)(postab + ((int64_t)blockIdx.y * S + s) * H + 256 * i + 4 * l) =
          make_float4(tot[i][0], tot[i][1], tot[i][2], tot[i][3]);
  }
  if (live && !DET) {  // this position's sum over the block's samples: position row, [CLS] / [SEP] word rows
               // (through the wave's LDS slice: lane-contiguous 256-B atomic instructions)
    const int64_t posr = text ? s - q.n_img - 2 : s;
    float* wr = s == 0 ? q.d_word + q.cls_id * H : (s == q.n_img + 1 ? q.d_word + q.sep_id * H : nullptr);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < NV; ++i)
      *(float4*)(&xch[wv][256 * i + 4 * l]) = make_float4(tot[i][0], tot[i][1], tot[i][2], tot[i][3]);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < 4 * NV; ++j) {
      const float v = xch[wv][64 * j + l];
      atomicAdd(q.d_pos + posr * H + 64 * j + l, v);
      if (wr) atomicAdd(wr + 64 * j + l, v);
    }
  }
#pragma unroll
  for (int half = 0; half < 2; ++half) {  // aw | ab, then type-0 | type-1
    if (half) __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = 256 * i + 4 * l + k;
        // token type 0: every image-segment row, text rows with seg 0
        red[0][wv][c] = half ? tot[i][k] - t1[i][k] : aw[i][k];
        red[1][wv][c] = half ? t1[i][k] : ab[i][k];
      }
    __syncthreads();
    for (int c = threadIdx.x; c < H; c += 256)
#pragma unroll
      for (int r = 0; r < 2; ++r)
        part[((2 * half + r) * nblk + blk) * H + c] = (red[r][0][c] + red[r][1][c]) + (red[r][2][c] + red[r][3][c]);
  }
}

int64_t embed_bwd_blocks(int64_t B, int64_t S) { return ((S + 3) / 4) * ((B + EBW_B - 1) / EBW_B); }

// ---------------------------------------------------------------- backward, deterministic mode
// d_word = a segmented sum over the text tokens sorted by id.  The pairs (id, flat row b T + t) are
// sorted by a stable LSD radix sort of the 32 key bits (the entry is not told the vocabulary), 8
// bits a pass: per tile of SORT_TILE keys one wave counts the digits (LDS integer counters), one
// block scans the [tiles][256] counts digit-major, and one wave per tile places its keys in index
// order (the rank among the wave's equal digits from ballots).  Stable, so the rows of one id
// ascend.  Nothing is allocated: pairs and counters lie in the workspace.
constexpr int SORT_TILE = 1024;
constexpr int EBW_DET_CHUNK = 64;  // tokens of the sorted sequence per wave of the segmented sum

template <bool FIRST>
__global__ __launch_bounds__(64) void sort_hist_kernel(const int64_t* __restrict__ ids,
                                                       const uint32_t* __restrict__ keys, int64_t n, int shift,
                                                       uint32_t* __restrict__ counts, int64_t ntile) {
  __shared__ uint32_t h[256];
  const int l = threadIdx.x;
  for (int d = l; d < 256; d += 64) h[d] = 0;
  __syncthreads();
  for (int st = 0; st < SORT_TILE / 64; ++st) {
    const int64_t i = (int64_t)blockIdx.x * SORT_TILE + st * 64 + l;
    if (i < n) {
      const uint32_t k = FIRST ? (uint32_t)ids[i] : keys[i];
      atomicAdd(&h[(k >> shift) & 255], 1u);
    }
  }
  __syncthreads();
  for (int d = l; d < 256; d += 64) counts[(int64_t)blockIdx.x * 256 + d] = h[d];
}

// exclusive scan of counts[tile][digit] in (digit, tile) order, in place: thread d walks its digit's
// column over the tiles (coalesced across the block), then adds the total of the smaller digits
__global__ __launch_bounds__(256) void sort_scan_kernel(uint32_t* __restrict__ counts, int64_t ntile) {
  __shared__ uint32_t tot[256];
  const int d = threadIdx.x;
  uint32_t run = 0;
#pragma unroll 8
  for (int64_t t = 0; t < ntile; ++t) run += counts[t * 256 + d];
  tot[d] = run;
  __syncthreads();
  uint32_t base = 0;
  for (int e = 0; e < d; ++e) base += tot[e];
#pragma unroll 8
  for (int64_t t = 0; t < ntile; ++t) {
    const uint32_t c = counts[t * 256 + d];
    counts[t * 256 + d] = base;
    base += c;
  }
}

template <bool FIRST>
__global__ __launch_bounds__(64) void sort_scatter_kernel(const int64_t* __restrict__ ids,
                                                          const uint32_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ vals, uint32_t* __restrict__ keys_out,
                                                          uint32_t* __restrict__ vals_out, int64_t n, int shift,
                                                          const uint32_t* __restrict__ counts, int64_t ntile) {
  __shared__ uint32_t base[256];
  const int l = threadIdx.x;
  for (int d = l; d < 256; d += 64) base[d] = counts[(int64_t)blockIdx.x * 256 + d];
  __syncthreads();
  for (int st = 0; st < SORT_TILE / 64; ++st) {
    const int64_t i = (int64_t)blockIdx.x * SORT_TILE + st * 64 + l;
    const bool valid = i < n;
    const uint32_t k = valid ? (FIRST ? (uint32_t)ids[i] : keys[i]) : 0u;
    const uint32_t v = valid ? (FIRST ? (uint32_t)i : vals[i]) : 0u;
    const uint32_t d = (k >> shift) & 255;
    uint64_t peers = __ballot(valid);  // the valid lanes holding this lane's digit
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = (d >> bit) & 1;
      const uint64_t m = __ballot(on);
      peers &= on ? m : ~m;
    }
    const int rank = __popcll(peers & ((1ull << l) - 1));
    if (valid) {
      const uint32_t dst = base[d] + rank;
      keys_out[dst] = k;
      vals_out[dst] = v;
    }
    __syncthreads();
    if (valid && rank == 0) base[d] += __popcll(peers);
    __syncthreads();
  }
}

// 4 consecutive floats of a gradient row: 16-B accesses where the caller's buffer allows them (the
// flat gradient store packs its tensors without padding), else four 4-B ones
static __device__ __forceinline__ float4 ld4(const float* p) {
  return ((uintptr_t)p & 15) == 0 ? *(const float4*)p : make_float4(p[0], p[1], p[2], p[3]);
}
static __device__ __forceinline__ void st4(float* p, float4 v) {
  if (((uintptr_t)p & 15) == 0) {
    *(float4*)p = v;
  } else {
    p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
  }
}
template <int NV>
static __device__ __forceinline__ void row_rmw(float* __restrict__ dst, const float (&acc)[NV][4], int l) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    float* d = dst + 256 * i + 4 * l;
    float4 o = ld4(d);
    o.x += acc[i][0]; o.y += acc[i][1]; o.z += acc[i][2]; o.w += acc[i][3];
    st4(d, o);
  }
}
template <int NV>
static __device__ __forceinline__ void row_store(float* __restrict__ dst, const float (&acc)[NV][4], int l) {
#pragma unroll
  for (int i = 0; i < NV; ++i)
    *(float4*)(dst + 256 * i + 4 * l) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
}

// First level of the segmented sum: one wave per chunk of EBW_DET_CHUNK sorted tokens walks them
// in order and sums each run of equal ids in registers.  A run that lies inside the chunk has this
// wave as its only writer: d_word[id] += sum.  A run that goes on from the previous chunk leaves
// its sum in carry row 0 of the chunk, one that begins here and goes on into the next chunk in
// carry row 1; embed_det_carry_kernel folds those.
template <int NV>
__global__ __launch_bounds__(64) void embed_det_chunk_kernel(const uint32_t* __restrict__ sk,
                                                             const uint32_t* __restrict__ sv, int64_t n,
                                                             const float* __restrict__ dxs, float* __restrict__ carry,
                                                             float* __restrict__ d_word) {
  constexpr int64_t H = 256 * NV;
  const int l = threadIdx.x;
  const int64_t c = blockIdx.x, c0 = c * EBW_DET_CHUNK;
  const int cnt = (int)(n - c0 < EBW_DET_CHUNK ? n - c0 : EBW_DET_CHUNK);
  const uint32_t my_k = l < cnt ? sk[c0 + l] : 0u, my_v = l < cnt ? sv[c0 + l] : 0u;
  const bool has_left = c0 > 0, has_right = c0 + cnt < n;
  const uint32_t left_k = has_left ? sk[c0 - 1] : 0u, right_k = has_right ? sk[c0 + cnt] : 0u;
  float acc[NV][4];
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[i][k] = 0.f;
  uint32_t cur = __shfl(my_k, 0, 64);
  bool first = true;
  for (int i = 0; i <= cnt; ++i) {
    const uint32_t k = __shfl(my_k, i < cnt ? i : 0, 64);
    if (i == cnt || k != cur) {  // the run of `cur` ends before token i
      const bool left_open = first && has_left && left_k == cur;
      const bool right_open = i == cnt && has_right && right_k == cur;
      if (left_open) row_store<NV>(carry + (2 * c) * H, acc, l);
      else if (right_open) row_store<NV>(carry + (2 * c + 1) * H, acc, l);
      else row_rmw<NV>(d_word + (int64_t)cur * H, acc, l);
      if (i == cnt) break;
#pragma unroll
      for (int a = 0; a < NV; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
      cur = k;
      first = false;
    }
    add_row<NV>(acc, dxs + (int64_t)__shfl(my_v, i, 64) * H, l);
  }
}

// Second level: the run that begins in chunk c and goes on past its end has one writer per 256
// columns here, which adds carry row 1 of c and then carry row 0 of every later chunk the run
// reaches, in chunk order, and d_word[id] += that sum.  The run's end is found by bisection of the
// sorted keys.
template <int NV>
__global__ __launch_bounds__(64) void embed_det_carry_kernel(const uint32_t* __restrict__ sk, int64_t n,
                                                             const float* __restrict__ carry,
                                                             float* __restrict__ d_word) {
  constexpr int64_t H = 256 * NV;  // gridDim.y == NV
  const int64_t c = blockIdx.x, c0 = c * EBW_DET_CHUNK, c1 = c0 + EBW_DET_CHUNK;
  if (c1 >= n) return;
  const uint32_t id = sk[c1 - 1];
  if (sk[c1] != id) return;                                // nothing goes on past this chunk
  if (sk[c0] == id && c0 > 0 && sk[c0 - 1] == id) return;  // the run began in an earlier chunk
  int64_t lo = c1, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (sk[mid] <= id) lo = mid + 1;
    else hi = mid;
  }
  const int64_t clast = (lo - 1) / EBW_DET_CHUNK;
  const int col = blockIdx.y * 256 + 4 * threadIdx.x;
  float4 a = *(const float4*)(carry + (2 * c + 1) * H + col);
#pragma unroll 8
  for (int64_t cc = c + 1; cc <= clast; ++cc) {
    const float4 v = *(const float4*)(carry + (2 * cc) * H + col);
    a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
  }
  float* d = d_word + (int64_t)id * H + col;
  float4 o = ld4(d);
  o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w;
  st4(d, o);
}

// Position rows and the [CLS] / [SEP] word rows from postab [nby, S, H], one writer each, the
// nby block rows folded in block order.  Block r < R: d_pos[r] += (the image-segment position r)
// then (the text position r).  Block R, after every token run of the launches before it:
// d_word[cls] += position 0's sum, then d_word[sep] += position n_img + 1's (one thread per
// column does both, so cls == sep stays ordered).
template <int NV>
__global__ __launch_bounds__(64) void embed_det_pos_kernel(const float* __restrict__ postab, int64_t nby, int64_t S,
                                                           int64_t T, int64_t n_img, int64_t R, int64_t cls_id,
                                                           int64_t sep_id, float* __restrict__ d_pos,
                                                           float* __restrict__ d_word) {
  constexpr int64_t H = 256 * NV;  // gridDim.y == NV
  const int col = blockIdx.y * 256 + 4 * threadIdx.x;
  const int64_t r = blockIdx.x;
  auto fold = [&](float* dst, int64_t s) {
    float4 a = ld4(dst + col);
    for (int64_t by = 0; by < nby; ++by) {
      const float4 v = *(const float4*)(postab + (by * S + s) * H + col);
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    st4(dst + col, a);
  };
  if (r < R) {
    if (r <= n_img + 1) fold(d_pos + r * H, r);
    if (r < T) fold(d_pos + r * H, n_img + 2 + r);
  } else {
    fold(d_word + cls_id * H, 0);
    fold(d_word + sep_id * H, n_img + 1);
  }
}

namespace {
struct DetLayout {  // offsets in floats behind the [4, nblk, H] partial rows; every section 16-B aligned
  int64_t n, nby, S, nch, ntile, n4;
  int64_t dxs, postab, carry, keys[2], vals[2], counts, total;
};
DetLayout det_layout(int64_t B, int64_t T, int64_t n_img, int64_t H) {
  DetLayout d{};
  d.n = B * T;
  d.nby = (B + EBW_B - 1) / EBW_B;
  d.S = n_img + 2 + T;
  d.nch = (d.n + EBW_DET_CHUNK - 1) / EBW_DET_CHUNK;
  d.ntile = (d.n + SORT_TILE - 1) / SORT_TILE;
  d.n4 = (d.n + 3) / 4 * 4;
  int64_t o = 0;
  d.dxs = o; o += d.n * H;
  d.postab = o; o += d.nby * d.S * H;
  d.carry = o; o += d.nch * 2 * H;
  for (int i = 0; i < 2; ++i) { d.keys[i] = o; o += d.n4; }
  for (int i = 0; i < 2; ++i) { d.vals[i] = o; o += d.n4; }
  d.counts = o; o += 256 * d.ntile;
  d.total = o;
  return d;
}
}  // namespace

int64_t embed_bwd_det_ws_floats(int64_t B, int64_t T, int64_t n_img, int64_t H) {
  return det_layout(B, T, n_img, H).total;
}
int64_t embed_bwd_det_chunk() { return EBW_DET_CHUNK; }

template <int NV>
static void embed_bwd_det_launch(const EmbedBwdParams& q, const EmbedParams& p, int64_t nblk, hipStream_t s) {
  constexpr int64_t H = 256 * NV;
  const DetLayout d = det_layout(q.B, q.T, q.n_img, H);
  float* base = q.ws + 4 * nblk * H;  // (dxs and postab: the rows kernel derives the same addresses)
  hipLaunchKernelGGL((embed_bwd_rows_kernel<NV, true>), dim3((unsigned)((p.Lout + 3) / 4), (unsigned)d.nby), dim3(256), 0, s,
                     q, p);
  if (d.n > 0) {
    uint32_t* keys[2] = {(uint32_t*)(base + d.keys[0]), (uint32_t*)(base + d.keys[1])};
    uint32_t* vals[2] = {(uint32_t*)(base + d.vals[0]), (uint32_t*)(base + d.vals[1])};
    uint32_t* counts = (uint32_t*)(base + d.counts);
    const dim3 tiles((unsigned)d.ntile);
    for (int pass = 0; pass < 4; ++pass) {  // pass 0 reads the ids; the sorted pairs end in keys[1] / vals[1]
      const int in = (pass + 1) & 1, out = pass & 1, shift = 8 * pass;
      if (pass == 0)
        hipLaunchKernelGGL(sort_hist_kernel<true>, tiles, dim3(64), 0, s, q.ids, (const uint32_t*)nullptr, d.n, shift,
                           counts, d.ntile);
      else
        hipLaunchKernelGGL(sort_hist_kernel<false>, tiles, dim3(64), 0, s, (const int64_t*)nullptr, keys[in], d.n,
                           shift, counts, d.ntile);
      hipLaunchKernelGGL(sort_scan_kernel, dim3(1), dim3(256), 0, s, counts, d.ntile);
      if (pass == 0)
        hipLaunchKernelGGL(sort_scatter_kernel<true>, tiles, dim3(64), 0, s, q.ids, (const uint32_t*)nullptr,
                           (const uint32_t*)nullptr, keys[out], vals[out], d.n, shift, counts, d.ntile);
      else
        hipLaunchKernelGGL(sort_scatter_kernel<false>, tiles, dim3(64), 0, s, (const int64_t*)nullptr, keys[in],
                           vals[in], keys[out], vals[out], d.n, shift, counts, d.ntile);
    }
    hipLaunchKernelGGL(embed_det_chunk_kernel<NV>, dim3((unsigned)d.nch), dim3(64), 0, s, keys[1], vals[1], d.n,
                       base + d.dxs, base + d.carry, q.d_word);
    if (d.nch > 1)
      hipLaunchKernelGGL(embed_det_carry_kernel<NV>, dim3((unsigned)d.nch, NV), dim3(64), 0, s, keys[1], d.n,
                         base + d.carry, q.d_word);
  }
  const int64_t R = q.n_img + 2 > q.T ? q.n_img + 2 : q.T;
  hipLaunchKernelGGL(embed_det_pos_kernel<NV>, dim3((unsigned)(R + 1), NV), dim3(64), 0, s, base + d.postab, d.nby, d.S,
                     q.T, q.n_img, R, q.cls_id, q.sep_id, q.d_pos, q.d_word);
}

template <int NV>
static void embed_bwd_launch_nv(const EmbedBwdParams& q, hipStream_t s) {
  constexpr int64_t H = 256 * NV;
  EmbedParams p{};
  p.ids = q.ids; p.seg = q.seg; p.txt_mask = nullptr; p.idx = nullptr;
  p.proj = q.proj; p.word = q.word; p.pos = q.pos; p.type = q.type;
  p.cls_id = q.cls_id; p.sep_id = q.sep_id; p.V = 1; p.B = q.B; p.T = q.T; p.n_img = q.n_img;
  p.Lout = q.n_img + 2 + q.T; p.H = H;
  const int64_t nblk = embed_bwd_blocks(q.B, p.Lout);
  if (deterministic())
    embed_bwd_det_launch<NV>(q, p, nblk, s);
  else
    hipLaunchKernelGGL((embed_bwd_rows_kernel<NV, false>), dim3((unsigned)((p.Lout + 3) / 4), (unsigned)((q.B + EBW_B - 1) / EBW_B)),
                       dim3(256), 0, s, q, p);
  const float* part = q.ws;
  ColsumJobs jobs{};
  float* outs[4] = {q.d_ln_w, q.d_ln_b, q.d_type, q.d_type + H};
  for (int z = 0; z < 4; ++z) {
    jobs.part[z] = part + z * nblk * H;
    jobs.parts[z] = nblk;
    jobs.out[z] = outs[z];
  }
  colsum_reduce_multi_launch(jobs, 4, H, 1, s);
}

void embed_bwd_launch(const EmbedBwdParams& q, hipStream_t s) {
  if (q.H == 1024) embed_bwd_launch_nv<4>(q, s);
  else embed_bwd_launch_nv<3>(q, s);
}

// ---------------------------------------------------------------- AdaptiveAvgPool2d((n,1))
// bin i covers rows [floor(i*Hh/n), ceil((i+1)*Hh/n)), all columns
__global__ __launch_bounds__(256) void row_pool_fwd_kernel(const bf16* __restrict__ f, int64_t B, int Hh, int Ww,
                                                           int64_t C, int n, float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;  // over B * C/8
  const int64_t c8 = C / 8;
  if (idx >= B * c8) return;
  const int64_t b = idx / c8, c = (idx % c8) * 8;
  for (int i = 0; i < n; ++i) {
    const int y0 = (i * Hh) / n, y1 = ((i + 1) * Hh + n - 1) / n;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int y = y0; y < y1; ++y)
      for (int x = 0; x < Ww; ++x) {
        bf16x8 v = *(const bf16x8*)(f + ((b * Hh + y) * Ww + x) * C + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += bf2f(v[e]);
      }
    const float inv = 1.0f / ((y1 - y0) * Ww);
    float* o = out + (b * n + i) * C + c;
    *(float4*)o = make_float4(acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv);
    *(float4*)(o + 4) = make_float4(acc[4] * inv, acc[5] * inv, acc[6] * inv, acc[7] * inv);
  }
}

__global__ __launch_bounds__(256) void row_pool_bwd_kernel(const float* __restrict__ d, int64_t B, int Hh, int Ww,
                                                           int64_t C, int n, bf16* __restrict__ df) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;  // over B*Hh * C/8
  const int64_t c8 = C / 8;
  if (idx >= B * Hh * c8) return;
  const int64_t by = idx / c8, c = (idx % c8) * 8, b = by / Hh;
  const int y = (int)(by % Hh);
  float g[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < n; ++i) {
    const int y0 = (i * Hh) / n, y1 = ((i + 1) * Hh + n - 1) / n;
    if (y < y0 || y >= y1) continue;
    const float inv = 1.0f / ((y1 - y0) * Ww);
    const float* s = d + (b * n + i) * C + c;
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] += s[e] * inv;
  }
  bf16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = f2bf(g[e]);
  for (int x = 0; x < Ww; ++x) *(bf16x8*)(df + ((b * Hh + y) * Ww + x) * C + c) = v;
}

void row_pool_fwd_launch(const bf16* fmap, int64_t B, int64_t Hh, int64_t Ww, int64_t C, int64_t n, float* out,
                         hipStream_t s) {
  const int64_t tot = B * (C / 8);
  hipLaunchKernelGGL(row_pool_fwd_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, fmap, B, (int)Hh,
                     (int)Ww, C, (int)n, out);
}
void row_pool_bwd_launch(const float* dout, int64_t B, int64_t Hh, int64_t Ww, int64_t C, int64_t n, bf16* dfmap,
                         hipStream_t s) {
  const int64_t tot = B * Hh * (C / 8);
  hipLaunchKernelGGL(row_pool_bwd_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, dout, B, (int)Hh,
                     (int)Ww, C, (int)n, dfmap);
}

}  // namespace mmu
