// Launch plans of the GEMM and conv products: everything the host decides before it launches --
// tiling, tile order, split-K, the split tail rows, the column-sum path -- as pure functions of the
// shape, the knobs and the scratch that can be had.  Plain C++: no HIP, no state, no environment,
// no allocation.  capi.hip executes a plan; mmu_gemm_plan / mmu_conv_implicit_plan /
// mmu_conv_wgrad_plan (include/mmu.h) report the same plan, also on a machine without a GPU.
//
// A plan function returns NULL, or the refusal that belongs to the plan: a printf format whose
// "%ld" arguments are the plan's `why` values, in order (fail(fmt, why[0], ..., why[5])).
#pragma once
#include <stdint.h>
#include "../../include/mmu.h"

namespace mmu {

// the CU count the tile-round heuristics assume (an MI355X; not the 256-row tile edge)
constexpr int64_t PLAN_CUS = 256;
// capacity of each per-stream scratch slot of mmu_gemm (the split tail's slabs, the column-sum
// partial rows): 32 MiB
constexpr int64_t TAIL_WS_FLOATS = 8ll << 20;

inline const char* refuse(int64_t (&why)[6], const char* fmt, int64_t a = 0, int64_t b = 0, int64_t c = 0,
                          int64_t d = 0, int64_t e = 0, int64_t f = 0) {
  why[0] = a; why[1] = b; why[2] = c; why[3] = d; why[4] = e; why[5] = f;
  return fmt;
}

// K in about `want` slices of whole 64-deep steps -> the slice depth; `slices` of it tile K
inline int64_t split_k(int64_t K, int64_t want, int& slices) {
  const int64_t chunk = ((K + want - 1) / want + 63) / 64 * 64;
  slices = (int)((K + chunk - 1) / chunk);
  return chunk;
}

// ------------------------------------------------------------------ mmu_gemm / mmu_gemm_rows
struct GemmShape {
  int64_t M, N, K, batch, lda, ldb;
  bool a_kmajor, b_kmajor, c_f32;
  int kind;  // MMU_EPI_*
  bool has_bias, has_colsum;
  int64_t ws_floats;  // the caller's split-K workspace (0: none)
};
struct GemmKnobs {
  int wide_mode = 1;              // MMU_GEMM_WIDE: 0 off, 1 the default rule, 2 every kind and width
  int64_t wide_min_tiles = 1024;  // MMU_GEMM_WIDE_MIN_TILES (default 4 per CU)
  int tail_mode = 1;              // MMU_GEMM_TAIL: 0 off, 1 on the wide tiling, 2 on 256 x 256 too
  int cs_part = 1;                // MMU_GEMM_CS_PART: 0 = column sums by float atomics
  bool deterministic = false;     // mmu_set_deterministic
};
struct GemmScratch {
  int64_t tail_floats, cs_floats;  // TAIL_WS_FLOATS each when the slot can be had, else 0
};
enum { GEMM_SMALL = 0, GEMM_BIG = 1, GEMM_WIDE = 2 };              // 128 x 128, 256 x 256, 256 x 384
enum { CS_NONE = 0, CS_ATOMICS = 1, CS_ROWS = 2, CS_TABLE = 3 };   // GemmPlan.cs
struct GemmPlan {
  int tiling, tiles_m, tiles_n;  // (tiles of the whole product, the tail rows included)
  int group_m;                   // tile-order group height (gemm.hip tile_of)
  int splitk;
  int64_t kchunk;
  // split tail rows: rows [m_main, M) run as tail_split slices of tail_chunk on the small tiling
  int64_t m_main, tail_rows;
  int tail_split;
  int64_t tail_chunk;
  // column sums.  CS_ROWS: cs_parts partial rows, one per cs_rows rows of the main tiling (64 of the tail)
  int cs, cs_rows;
  int64_t cs_parts;
  int64_t why[6];
};

// the kinds the split tail's epilogue kernel (splitk_epilogue_launch) and the 256 x 384 kernel
// (gemm_wide_launch) are instantiated for
inline bool gemm_tail_kind(int kind) {
  return kind == MMU_EPI_STORE || kind == MMU_EPI_BIAS_GELU || kind == MMU_EPI_BIAS_DROP_RES ||
         kind == MMU_EPI_DGELU || kind == MMU_EPI_ADD_RES;
}

inline const char* gemm_plan(const GemmShape& g, const GemmKnobs& kn, const GemmScratch& sc, GemmPlan& pl) {
  const int64_t M = g.M, N = g.N, K = g.K, batch = g.batch;
  const int kind = g.kind;
  pl = GemmPlan{};
  if (M <= 0 || N <= 0 || K <= 0 || batch <= 0) return refuse(pl.why, "mmu_gemm: bad shape M=%ld N=%ld K=%ld", M, N, K);
  if (N % 128) return refuse(pl.why, "mmu_gemm: N=%ld must be a multiple of 128", N);
  if ((g.a_kmajor || g.b_kmajor) && K % 64)
    return refuse(pl.why, "mmu_gemm: K=%ld must be a multiple of 64 for a K-major operand", K);
  if (!g.a_kmajor && M % 128) return refuse(pl.why, "mmu_gemm: M=%ld must be a multiple of 128 when A is M-major", M);
  // big (256x256, LDS-DMA) tiling needs >= 256 rows/cols and 32-bit buffer offsets per operand
  // (spans include the rows a 256-tile / 64-deep K-tile may address past the end, so the
  // 32-bit buffer offsets of those out-of-range reads never wrap back into the operand)
  const int64_t span_max = (1ll << 32) - 4096;
  const int64_t a_span = 2 * (g.a_kmajor ? (M + 256) * g.lda : (K + 64) * g.lda);
  const int64_t b_span = 2 * (g.b_kmajor ? (N + 256) * g.ldb : (K + 64) * g.ldb);
  const bool big = M >= 256 && N >= 256 && a_span < span_max && b_span < span_max;
  const int tile = big ? 256 : 128;
  pl.tiles_m = (int)((M + tile - 1) / tile);
  pl.tiles_n = (int)((N + tile - 1) / tile);
  // tile-order group height, measured on the BERT shapes (tools/gemm_bench.py; group-height
  // sweeps in profiles/r1_gemm_group_sweep.txt): row-major for <= 3 column tiles, 2 with an N-major B (dY.W2), 8 for the
  // wide forward products (QKV 0.496 -> 0.457 ms, W1+GELU 0.888 -> 0.832 ms)
  // (and 2 for the dGELU product dY2.W2, whose epilogue streams the [M, 3072] gelu' rows:
  // 0.888 -> 0.756 ms with a K-major B, profiles/r2_gemm_group_dz.txt)
  pl.group_m = pl.tiles_n <= 3 ? 1 : ((g.b_kmajor && kind != MMU_EPI_DGELU) ? 8 : 2);
  // split-K for long-K / few-tile products (the weight gradients: K = tokens, M x N = a weight matrix)
  pl.splitk = 1;
  pl.kchunk = K;
  if (kind == MMU_EPI_STORE && g.c_f32 && !g.has_bias && !g.has_colsum && g.ws_floats > 0 && K >= 1024) {
    const int64_t tiles = (int64_t)pl.tiles_m * pl.tiles_n * batch;
    // slice cap 64 / minimum slice depth 1024 (profiles/r2_splitk_cap_ab.txt); short reductions
    // (the batch-32 ResNet filter gradients: K = 1.5-25 K pixels over 4-16 tiles) go down to
    // 256-deep slices so that they still fill the chip
    const int64_t max_split = 64, min_k = K >= 32768 ? 1024 : 256;
    int64_t want = (640 + tiles - 1) / tiles;
    if (want > K / min_k) want = K / min_k;
    if (want > max_split) want = max_split;
    const int64_t cap = g.ws_floats / (batch * M * N);
    if (want > cap) want = cap;
    if (want >= 2) pl.kchunk = split_k(K, want, pl.splitk);
  }
  // 256 x 384 tiling (gemm_wide_kernel): both operands K-major, N % 384 == 0, no split-K, and at
  // least wide_min_tiles of its tiles (default 4 per CU: the bench's M = 131 k rows; fewer, larger
  // tiles leave CUs idle on small products).
  // (the dGELU product stays on 256 x 256: its aux-row loads and column-sum atomics per 64-row
  // block ran it 15-22 % slower on the wide tile, profiles/r6_gemm_wide_ab.txt)
  const bool tail_kind = gemm_tail_kind(kind);
  const bool wide_kind = tail_kind && kind != MMU_EPI_DGELU;
  // Default rule (wide_mode 1), same-box A/B: the wide products N >= 2304 (QKV -3 %, FFN1 + GELU
  // -8 % with the split tail); N = 768 stays on 256 x 256 (equal or 2 % slower: its 1026 wide tiles
  // end in a round of 2).  wide_mode 2 takes every kind and width (tests).
  const bool wide = (kn.wide_mode == 2 ? tail_kind : kn.wide_mode == 1 && wide_kind && N >= 2304) && big &&
                    g.a_kmajor && g.b_kmajor && N % 384 == 0 && pl.splitk == 1 &&
                    2 * (M + 256) * g.lda < span_max && 2 * (N + 384) * g.ldb < span_max &&
                    (M + 255) / 256 * (N / 384) * batch >= kn.wide_min_tiles;
  if (wide) {
    pl.tiles_m = (int)((M + 255) / 256);
    pl.tiles_n = (int)(N / 384);
    pl.group_m = pl.tiles_n <= 2 ? 1 : (kind != MMU_EPI_DGELU ? 8 : 2);
  }
  pl.tiling = wide ? GEMM_WIDE : big ? GEMM_BIG : GEMM_SMALL;
  // Split tail rows: when the last round of 256-row tiles holds whole tile rows and is at most an
  // eighth full (M = 256 x 513 at batch 256: 1026 wide / 1539 big tiles on 256 CUs), those rows
  // run as split-K partial products of the small tiling into a per-stream f32 scratch, and
  // splitk_epilogue_kernel sums them and applies the same epilogue.  On by default for the wide
  // tiling (tail_mode 1), whose tail round is 1.5 big tiles long; 2 = for the 256 x 256 tiling
  // too (tests: there it costs +10-20 us, the 256^2 tail round is short), 0 = off.
  pl.m_main = M;
  pl.tail_rows = 0;
  pl.tail_split = 1;
  pl.tail_chunk = K;
  if ((kn.tail_mode == 2 || (kn.tail_mode == 1 && wide)) && big && batch == 1 && pl.splitk == 1 && tail_kind &&
      g.a_kmajor && K >= 512) {
    const int64_t tiles = (int64_t)pl.tiles_m * pl.tiles_n, left = tiles % PLAN_CUS;
    if (tiles > PLAN_CUS && left > 0 && left % pl.tiles_n == 0 && left * 8 <= PLAN_CUS) {
      const int64_t m_main = (int64_t)(pl.tiles_m - left / pl.tiles_n) * 256, rows = M - m_main;
      const int64_t st = (rows + 127) / 128 * (N / 128);  // small tiles over the tail rows
      int64_t sk = PLAN_CUS / st;
      if (sk > K / 256) sk = K / 256;  // >= 4 K-steps per slice
      if (sk < 1) sk = 1;
      int split;
      const int64_t chunk = split_k(K, sk, split);
      // (a single slice would make the small kernel store its raw product into C: no split then)
      if (split >= 2 && (int64_t)split * rows * N <= sc.tail_floats) {
        pl.m_main = m_main;
        pl.tail_rows = rows;
        pl.tail_split = split;
        pl.tail_chunk = chunk;
      }
    }
  }
  // column sums as partial rows (no float atomics: 50 us of the 0.74 ms dZ product at batch 256,
  // 180 us on the wide tile; profiles/r6_gemm_colsum_ab.txt), folded by one colsum_reduce launch.
  // Rows of 16 NJ per wave block: 128 on the 256 x 256 tile, 64 on the others.  cs_part 0: atomics.
  // Deterministic mode: always the partial rows, whatever cs_part says; a plain colsum that
  // cannot take them (batch > 1, no scratch) is refused instead of reaching the atomics.
  const bool table = kind == MMU_EPI_STORE_STATS || kind == MMU_EPI_STORE_BNB || kind == MMU_EPI_ADD_RES_BNB;
  pl.cs = !g.has_colsum ? CS_NONE : table ? CS_TABLE : CS_ATOMICS;
  if (pl.cs == CS_ATOMICS) {
    const bool rows_ok = batch == 1 && pl.splitk == 1 && (kn.deterministic || kn.cs_part != 0);
    const int cs_rows = (big && !wide) ? 128 : 64;
    const int64_t parts = (pl.m_main + cs_rows - 1) / cs_rows + (pl.tail_rows + 63) / 64;
    if (rows_ok && parts * N <= sc.cs_floats) {
      pl.cs = CS_ROWS;
      pl.cs_rows = cs_rows;
      pl.cs_parts = parts;
    } else if (kn.deterministic) {
      return refuse(pl.why,
                    rows_ok ? "mmu_gemm: deterministic mode: colsum with batch=%ld splitk=%ld has no partial-row path"
                              " (no scratch: table too large, or first use under stream capture)"
                            : "mmu_gemm: deterministic mode: colsum with batch=%ld splitk=%ld has no partial-row path",
                    batch, pl.splitk);
    }
  }
  return nullptr;
}

// ------------------------------------------------------------------ the gathered conv products
// ksize 3 (pad 1) or 1 (pad 0), stride 1..4, over an NHWC map [n, H, W, C]
struct ConvShape {
  int64_t n, H, W, C, N, ksize, stride;  // C -> N channels (the weight gradient: Cin -> Cout)
  int64_t ws_floats;                     // the caller's split-K workspace (0: none)
};
struct ConvPlan {
  int64_t Ho, Wo, pixels;  // pixels = n Ho Wo: the forward's M, the weight gradient's K
  int64_t K;               // the contraction depth: ksize^2 C taps x channels, or the pixels
  int64_t in_bytes;        // the input map, for the gather's buffer bounds
  bool small;              // forward: 128 x 128 register-staged tiles (else 256 x 256, LDS-DMA gather)
  bool few;                // weight gradient: <= 4 output tiles
  int tiles_m, tiles_n, splitk;
  int64_t kchunk;
  int64_t why[6];
};

// -> 0, 1 (bad geometry) or 2 (the map too large)
inline int conv_geometry(const ConvShape& c, ConvPlan& pl) {
  if (c.n <= 0 || c.H <= 0 || c.W <= 0 || c.C <= 0 || (c.ksize != 1 && c.ksize != 3) || c.stride < 1 || c.stride > 4) {
    refuse(pl.why, nullptr, c.n, c.H, c.W, c.C, c.ksize, c.stride);
    return 1;
  }
  const int64_t pad = c.ksize / 2;
  pl.Ho = (c.H + 2 * pad - c.ksize) / c.stride + 1;
  pl.Wo = (c.W + 2 * pad - c.ksize) / c.stride + 1;
  pl.pixels = c.n * pl.Ho * pl.Wo;
  pl.in_bytes = 2 * c.n * c.H * c.W * c.C;
  return pl.in_bytes >= 0x7FFF0000ll ? 2 : 0;
}

// forward / data gradient: Y [pixels][N] = im2col(X) [pixels][T C] . Wk^T
inline const char* conv_implicit_plan(const ConvShape& c, ConvPlan& pl) {
  pl = ConvPlan{};
  if (c.C % 64 || c.N % 64 || c.N <= 0)
    return refuse(pl.why, "mmu_conv_implicit: needs C %% 64 == 0, N %% 64 == 0 (C=%ld N=%ld)", c.C, c.N);
  switch (conv_geometry(c, pl)) {
    case 1: return "mmu_conv_implicit: bad geometry (n=%ld H=%ld W=%ld C=%ld ksize=%ld stride=%ld)";
    case 2: return "mmu_conv_implicit: input map too large for 32-bit buffer offsets";
  }
  const int64_t M = pl.pixels, N = c.N, K = pl.K = c.ksize * c.ksize * c.C;
  if (M < 256 || 2 * (M + 256) * N >= (1ll << 31) || 2 * (N + 256) * K >= (1ll << 31))
    return "mmu_conv_implicit: map size out of range";
  // 256x256 tiles (LDS-DMA gather) for N >= 256 with N % 128 == 0; 128x128 register-staged
  // tiles for the narrow convs (N = 64 / 128 / ...)
  pl.small = N < 256 || N % 128;
  const int tile = pl.small ? 128 : 256;
  pl.tiles_m = (int)((M + tile - 1) / tile);
  pl.tiles_n = (int)((N + tile - 1) / tile);
  pl.splitk = 1;
  pl.kchunk = K;
  // split K (taps x channels) when the map has fewer tiles than half the CUs: ~512 blocks, >= 4
  // 64-deep steps per slice, slabs bounded by the workspace
  const int64_t tiles = (int64_t)pl.tiles_m * pl.tiles_n;
  if (c.ws_floats > 0 && tiles < PLAN_CUS / 2) {
    int64_t want = (512 + tiles - 1) / tiles;
    if (want > K / 256) want = K / 256;
    if (want > c.ws_floats / (M * N)) want = c.ws_floats / (M * N);
    if (want >= 2) pl.kchunk = split_k(K, want, pl.splitk);
  }
  return nullptr;
}

// weight gradient: dW [Cout][T Cin] = dY^T [Cout][pixels] . im2col(X) [pixels][T Cin]
inline const char* conv_wgrad_plan(const ConvShape& c, ConvPlan& pl) {
  pl = ConvPlan{};
  const int64_t Cin = c.C, Cout = c.N;
  if (Cin % 256 || Cout % 128 || Cin <= 0 || Cout <= 0)
    return refuse(pl.why, "mmu_conv_wgrad: needs Cin %% 256 == 0, Cout %% 128 == 0 (Cin=%ld Cout=%ld)", Cin, Cout);
  switch (conv_geometry(c, pl)) {
    case 1: return "mmu_conv_wgrad: bad geometry (n=%ld H=%ld W=%ld C=%ld ksize=%ld stride=%ld)";
    case 2: return "mmu_conv_wgrad: input map too large for 32-bit buffer offsets";
  }
  const int64_t K = pl.K = pl.pixels, N = c.ksize * c.ksize * Cin;
  if (K >= (1 << 24) || 2 * (K + 64) * Cout >= (1ll << 31))
    return "mmu_conv_wgrad: map too large for 32-bit buffer offsets";
  pl.tiles_m = (int)((Cout + 255) / 256);
  pl.tiles_n = (int)(N / 256);
  // split-K over the pixels (few output tiles): ~640 blocks, >= 1024 pixels per slice
  const int64_t tiles = (int64_t)pl.tiles_m * pl.tiles_n;
  int64_t want = (640 + tiles - 1) / tiles;
  // (the 2-tile 1x1 downsample, Cin 256 -> Cout 512: up to 128 slices of >= 256 pixels)
  pl.few = tiles <= 4;
  if (want > K / (pl.few ? 256 : 1024)) want = K / (pl.few ? 256 : 1024);
  if (want > (pl.few ? 128 : 32)) want = pl.few ? 128 : 32;
  const int64_t cap = c.ws_floats > 0 ? c.ws_floats / (Cout * N) : 0;
  if (want > cap) want = cap;
  pl.splitk = 1;
  pl.kchunk = K;
  if (want >= 2) pl.kchunk = split_k(K, want, pl.splitk);
  return nullptr;
}

}  // namespace mmu
