// Exact rank table over many score columns (gfx950): include/mmu.h mmu_rank_table.
//
// Every ranking metric of the analyses (AUROC with its tie rule, the area under the risk-coverage
// curve) is a function of, per sample, how many samples of each group score lower and how many score
// the same.  This kernel counts them by the all-pairs sweep, O(S^2) IEEE f32 compares per column, and
// the host forms every figure in fp64 from the integers (src/ranking.py).
//
// Grid (ceil(S / RK_ROWS), J), one 4-wave block per RK_ROWS samples of one column.  A lane keeps RK_R
// samples in registers with four int counters each.  The column's S candidates stream through LDS in
// tiles of RK_TILE values plus their group bytes; all lanes read the same LDS address per step (a
// broadcast, no bank conflict), four candidates per ds_read_b128.  The candidate is the same for every
// lane, so its group is read into a scalar register and the branch on it is wave-uniform.  Tile tails
// are padded with NaN, which counts nowhere -- by the rule that keeps real NaNs out.
// The column sums are 64-bit integer atomic adds of one value per block onto the zeroed counts: an
// integer sum does not depend on its order, so the result is bitwise repeatable, and the same launch
// serves both determinism modes.  No float is ever added.
#include <cmath>
#include "mmu_internal.h"

namespace mmu {

constexpr int RK_WAVES = 4;
constexpr int RK_THREADS = 64 * RK_WAVES;
constexpr int RK_R = 4;                      // samples per lane
constexpr int RK_ROWS = RK_THREADS * RK_R;   // samples per block (mmu.h MMU_RANK_BLOCK_ROWS)
constexpr int RK_TILE = 1024;                // candidates per LDS tile (mmu.h MMU_RANK_TILE)
static_assert(RK_ROWS == MMU_RANK_BLOCK_ROWS && RK_TILE == MMU_RANK_TILE, "mmu.h states the kernel's tiling");
static_assert(RK_TILE % RK_THREADS == 0 && RK_TILE % 4 == 0, "the tile is loaded by whole rounds of the block");

static __device__ __forceinline__ long long rk_wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(RK_THREADS) void rank_table_kernel(const float* __restrict__ x, int64_t ss, int64_t sj,
                                                                const uint8_t* __restrict__ group, int S,
                                                                int32_t* __restrict__ rank,
                                                                unsigned long long* __restrict__ counts) {
  __shared__ __attribute__((aligned(16))) float sv[RK_TILE];
  __shared__ __attribute__((aligned(4))) uint8_t sg[RK_TILE];
  __shared__ long long part[RK_WAVES][MMU_RANK_NCOUNT];

  const int tid = threadIdx.x;
  const int j = blockIdx.y;
  const float* xj = x + (int64_t)j * sj;
  const int row0 = blockIdx.x * RK_ROWS;

  float mine[RK_R];
  int lt0[RK_R], eq0[RK_R], lt1[RK_R], eq1[RK_R];
#pragma unroll
  for (int r = 0; r < RK_R; ++r) {
    const int i = row0 + r * RK_THREADS + tid;
    mine[r] = i < S ? xj[(int64_t)i * ss] : NAN;   // a row past the end compares false with everything
    lt0[r] = eq0[r] = lt1[r] = eq1[r] = 0;
  }

  for (int t0 = 0; t0 < S; t0 += RK_TILE) {
    __syncthreads();   // the previous tile has been read by every wave
#pragma unroll
    for (int k = 0; k < RK_TILE / RK_THREADS; ++k) {
      const int c = k * RK_THREADS + tid;
      const int i = t0 + c;
      sv[c] = i < S ? xj[(int64_t)i * ss] : NAN;
      sg[c] = i < S ? (uint8_t)(group[i] != 0) : (uint8_t)0;
    }
    __syncthreads();
    const int n = min(RK_TILE, (S - t0 + 3) & ~3);   // whole groups of four; the tail of the last is NaN
    for (int c = 0; c < n; c += 4) {
      const float4 v4 = *reinterpret_cast<const float4*>(&sv[c]);
      const uint32_t g4 = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const uint32_t*>(&sg[c]));
      const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if ((g4 >> (8 * q)) & 0xffu) {
#pragma unroll
          for (int r = 0; r < RK_R; ++r) {
            lt1[r] += v[q] < mine[r] ? 1 : 0;
            eq1[r] += v[q] == mine[r] ? 1 : 0;
          }
        } else {
#pragma unroll
          for (int r = 0; r < RK_R; ++r) {
            lt0[r] += v[q] < mine[r] ? 1 : 0;
            eq0[r] += v[q] == mine[r] ? 1 : 0;
          }
        }
      }
    }
  }

  long long sum[MMU_RANK_NCOUNT] = {0, 0, 0, 0, 0};
#pragma unroll
  for (int r = 0; r < RK_R; ++r) {
    const int i = row0 + r * RK_THREADS + tid;
    if (i >= S) continue;
    if (rank) {
      int32_t* o = rank + ((int64_t)j * S + i) * MMU_RANK_NRANK;
      o[MMU_RANK_LT0] = lt0[r];
      o[MMU_RANK_EQ0] = eq0[r];
      o[MMU_RANK_LT1] = lt1[r];
      o[MMU_RANK_EQ1] = eq1[r];
    }
    if (mine[r] != mine[r]) {
      sum[MMU_RANK_NAN] += 1;
    } else if (group[i] != 0) {
      sum[MMU_RANK_N1] += 1;
      sum[MMU_RANK_GT] += lt0[r];
      sum[MMU_RANK_EQ] += eq0[r];
    } else {
      sum[MMU_RANK_N0] += 1;
    }
  }
#pragma unroll
  for (int q = 0; q < MMU_RANK_NCOUNT; ++q) {
    const long long w = rk_wave_sum(sum[q]);
    if ((tid & 63) == 0) part[tid >> 6][q] = w;
  }
  __syncthreads();
  if (tid < MMU_RANK_NCOUNT) {
    long long tot = 0;
#pragma unroll
    for (int w = 0; w < RK_WAVES; ++w) tot += part[w][tid];
    if (tot) atomicAdd(&counts[(int64_t)j * MMU_RANK_NCOUNT + tid], (unsigned long long)tot);
  }
}

hipError_t rank_table_launch(const float* x, int64_t ss, int64_t sj, const uint8_t* group, int64_t S, int64_t J,
                             int32_t* rank, int64_t* counts, hipStream_t s) {
  const hipError_t e = hipMemsetAsync(counts, 0, (size_t)J * MMU_RANK_NCOUNT * sizeof(int64_t), s);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)((S + RK_ROWS - 1) / RK_ROWS), (unsigned)J);
  rank_table_kernel<<<grid, RK_THREADS, 0, s>>>(x, ss, sj, group, (int)S, rank,
                                                reinterpret_cast<unsigned long long*>(counts));
  return hipSuccess;
}

}  // namespace mmu
