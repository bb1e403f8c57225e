// Exact, deterministic top-k for 1 <= k <= 1024 per row of a dense fp32 block
// (tt_topk_rows; behind tt_search_topk / tt_hardneg_topk for k > 16, where the per-lane
// sorted lists of tt_topk.h do not stretch). Ordering as ttk::better: value descending,
// ties towards the lower column; -0.0 and +0.0 are equal.
//
// One workgroup per (row, column chunk) holds the chunk's keys in LDS and
//   1. maps each value to an order-preserving uint32 key (-0.0 folded onto +0.0),
//   2. radix-selects the kk-th largest key T (kk = min(k, chunk length)): four passes of
//      8-bit digits, a 256-bin LDS histogram each (integer atomics: counts do not depend
//      on order), the digit found by a suffix scan over the bins,
//   3. compacts, walking the chunk in index order: every key > T, and of the keys == T
//      exactly the first `need` (64-bit ballots + lane-mask popcounts inside a wave, the
//      waves' counts through LDS, the running counts carried from tile to tile),
//   4. at the last level, bitonic-sorts the k composites (key << 32 | ~index) descending in
//      LDS, padded to a power of two with 0, which sorts last (key 0 is a NaN pattern,
//      ~index 0 no column), and writes idx and the stored values.
// A row longer than one chunk runs in levels: every chunk emits its kk composites (keys > T
// in index order, then the chosen keys == T in index order; unsorted, since the next level
// selects again), and the same kernel selects from that list (explicit indices) until one
// chunk is left. Within a list, equal keys stand in ascending column order: inside one
// chunk's output they are all in the first part or all in the second, each in index order;
// chunks follow in column order; later levels cut the lists at multiples of k, between
// chunk outputs. So "the first `need` in list order" is the tie rule at every level. Every
// list slot that a level reads was written by the level before: nothing depends on the
// workspace's contents.
#include <climits>

#include "tt_api.h"
#include "tt_common.h"
#include "tt_topk.h"

namespace {

constexpr int SEL_CH = 8192;  // keys per workgroup: 32 KiB of LDS, 8 x the largest k
constexpr int SEL_THREADS = 512;
constexpr int SEL_WAVES = SEL_THREADS / 64;
static_assert(SEL_THREADS >= 256, "the first 256 threads own the histogram's bins");
constexpr int SEL_LEVELS = 12;

TT_DEV uint32_t sel_key(float v) {
  uint32_t u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// FIRST: keys from S[row, p0 .. p0 + m) with column label_off + row reading -1;
// else from the composites in[row * in_stride + p0 ..). idx != nullptr: the last level
// (one chunk per row), writes idx / val [rows, k]; else composites to out.
template <bool FIRST>
__global__ __launch_bounds__(SEL_THREADS) void select_kernel(const float* __restrict__ S, long ld, long label_off,
                                                             const uint64_t* __restrict__ in, long in_stride, long n,
                                                             int chunk, int nch, int k, uint64_t* __restrict__ out,
                                                             int32_t* __restrict__ idx, float* __restrict__ val) {
  __shared__ uint32_t s_key[SEL_CH];
  __shared__ uint64_t s_sel[ttk::SEL_MAX];
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_wsum[4];
  __shared__ uint32_t s_pick[2];
  __shared__ uint32_t s_cnt[2][SEL_WAVES][2];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long row = blockIdx.x / nch;
  const int j = blockIdx.x % nch;
  const long p0 = (long)j * chunk;
  const int m = (int)(n - p0 < chunk ? n - p0 : chunk);
  const int kk = k < m ? k : m;
  const long lab = label_off >= 0 ? label_off + row : -1;
  const float* srow = S + row * ld;
  const uint64_t* irow = FIRST ? nullptr : in + row * in_stride + p0;

  for (int i = tid; i < m; i += SEL_THREADS) {
    if constexpr (FIRST) s_key[i] = sel_key(p0 + i == lab ? -1.f : srow[p0 + i]);
    else s_key[i] = (uint32_t)(irow[i] >> 32);
  }

  // T = the kk-th largest key; need = how many of the keys == T belong to the top kk
  uint32_t prefix = 0, mask = 0;
  int need = kk;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) s_hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < m; i += SEL_THREADS) {
      const uint32_t key = s_key[i];
      if ((key & mask) == prefix) atomicAdd(&s_hist[(key >> shift) & 255], 1u);
    }
    __syncthreads();
    // the first four waves scan the bins from the top: inc = keys of this digit or a larger one
    const int bin = 255 - tid;
    uint32_t v = 0, inc = 0;
    if (tid < 256) {
      v = s_hist[bin];
      inc = v;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
      }
      if (lane == 63) s_wsum[wave] = inc;
    }
    __syncthreads();
    if (tid < 256) {
      for (int w = 0; w < wave; ++w) inc += s_wsum[w];
      const uint32_t exc = inc - v;
      if (exc < (uint32_t)need && (uint32_t)need <= inc) {
        s_pick[0] = (uint32_t)bin;
        s_pick[1] = (uint32_t)need - exc;
      }
    }
    __syncthreads();
    prefix |= s_pick[0] << shift;
    mask |= 0xFFu << shift;
    need = (int)s_pick[1];
  }

  const uint32_t T = prefix;
  const int ngt = kk - need;
  const uint64_t lt = (1ull << lane) - 1;
  int cg = 0, ce = 0;  // keys > T and == T before this tile
  for (int base = 0, it = 0; base < m; base += SEL_THREADS, ++it) {
    const int i = base + tid;
    const uint32_t key = i < m ? s_key[i] : 0u;
    const bool gt = i < m && key > T, eq = i < m && key == T;
    const uint64_t bg = __ballot(gt), be = __ballot(eq);
    uint32_t(*cnt)[2] = s_cnt[it & 1];
    if (lane == 0) {
      cnt[wave][0] = (uint32_t)__popcll(bg);
      cnt[wave][1] = (uint32_t)__popcll(be);
    }
    __syncthreads();
    int pg = cg + __popcll(bg & lt), pe = ce + __popcll(be & lt);
#pragma unroll
    for (int w = 0; w < SEL_WAVES; ++w) {
      const int g = (int)cnt[w][0], e = (int)cnt[w][1];
      if (w < wave) { pg += g; pe += e; }
      cg += g;
      ce += e;
    }
    if (gt || (eq && pe < need)) {
      uint64_t c;
      if constexpr (FIRST) c = ((uint64_t)key << 32) | (uint32_t)~(uint32_t)(p0 + i);
      else c = irow[i];
      s_sel[gt ? pg : ngt + pe] = c;
    }
  }

  if (!idx) {  // not the last level: the next one selects again and needs only the tie order
    __syncthreads();
    uint64_t* o = out + (row * nch + j) * k;
    for (int q = tid; q < kk; q += SEL_THREADS) o[q] = s_sel[q];
    return;
  }

  int P = 1;
  while (P < kk) P <<= 1;
  for (int i = kk + tid; i < P; i += SEL_THREADS) s_sel[i] = 0;
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < P / 2; t += SEL_THREADS) {
        const int a = 2 * t - (t & (stride - 1)), b = a + stride;
        const uint64_t x = s_sel[a], y = s_sel[b];
        if ((x < y) == ((a & size) == 0)) {
          s_sel[a] = y;
          s_sel[b] = x;
        }
      }
      __syncthreads();
    }
  }

  for (int q = tid; q < kk; q += SEL_THREADS) {
    const uint32_t col = ~(uint32_t)s_sel[q];
    idx[row * k + q] = (int32_t)col;
    if (val) val[row * k + q] = (long)col == lab ? -1.f : srow[col];
  }
}

// Level l reads n[l] entries per row in nch[l] chunks of chunk[l]; the last level has one chunk.
struct SelPlan {
  int levels;
  long n[SEL_LEVELS];
  int chunk[SEL_LEVELS], nch[SEL_LEVELS];
  long buf[2];  // bytes of the two composite lists the levels alternate between
};

inline long al256(long x) { return (x + 255) & ~255L; }

inline bool sel_plan(long rows, long cols, int k, SelPlan& p) {
  p = SelPlan{};
  long n = cols;
  int chunk = SEL_CH;
  // short of workgroups for the chip: narrower first-level chunks, still several times k wide
  while (cols > SEL_CH && chunk / 2 >= 4 * k && chunk / 2 >= 1024 && rows * ((cols + chunk - 1) / chunk) < 1024)
    chunk /= 2;
  for (int l = 0; l < SEL_LEVELS; ++l) {
    const long nch = (n + chunk - 1) / chunk;
    if (rows * nch > INT_MAX) return false;
    p.n[l] = n;
    p.chunk[l] = chunk;
    p.nch[l] = (int)nch;
    p.levels = l + 1;
    if (nch == 1) return true;
    const long bytes = al256(rows * nch * k * 8);
    if (bytes > p.buf[l & 1]) p.buf[l & 1] = bytes;
    const long last = n - (nch - 1) * chunk;
    n = (nch - 1) * k + (last < k ? last : k);
    chunk = SEL_CH / k * k;  // lists are cut between the chunk outputs of the level before
  }
  return false;
}

}  // namespace

extern "C" int tt_topk_max(void) { return ttk::SEL_MAX; }

extern "C" long tt_topk_rows_ws_size(long rows, long cols, int k) {
  SelPlan p;
  if (rows <= 0 || cols <= 0 || k < 1 || k > ttk::SEL_MAX || k > cols || !sel_plan(rows, cols, k, p)) return 0;
  return p.buf[0] + p.buf[1];
}

extern "C" int tt_topk_rows(const float* S, long rows, long cols, long ld, long label_offset, int k, int32_t* idx,
                            float* val, void* ws, void* stream) {
  TT_CHECK_ARG(k >= 1 && k <= ttk::SEL_MAX && k <= cols, "tt_topk_rows: k=%d needs 1 <= k <= min(%d, cols=%ld)", k,
               ttk::SEL_MAX, cols);
  TT_CHECK_ARG(rows >= 0 && cols <= INT_MAX && ld >= cols, "tt_topk_rows: rows=%ld cols=%ld ld=%ld", rows, cols, ld);
  if (rows == 0) return 0;
  TT_CHECK_ARG(S && idx, "tt_topk_rows: null S or idx");
  SelPlan p;
  TT_CHECK_ARG(sel_plan(rows, cols, k, p), "tt_topk_rows: rows=%ld x cols=%ld is too many chunks", rows, cols);
  TT_CHECK_ARG(p.levels == 1 || ws, "tt_topk_rows: needs a workspace (tt_topk_rows_ws_size)");
  hipStream_t st = (hipStream_t)stream;
  uint64_t* buf[2] = {static_cast<uint64_t*>(ws), reinterpret_cast<uint64_t*>(static_cast<char*>(ws) + p.buf[0])};
  const uint64_t* in = nullptr;
  long in_stride = 0;
  for (int l = 0; l < p.levels; ++l) {
    const bool last = l == p.levels - 1;
    uint64_t* out = last ? nullptr : buf[l & 1];
    const dim3 grid((unsigned)(rows * p.nch[l]));
    if (l == 0)
      hipLaunchKernelGGL(select_kernel<true>, grid, dim3(SEL_THREADS), 0, st, S, ld, label_offset, in, in_stride,
                         p.n[l], p.chunk[l], p.nch[l], k, out, last ? idx : nullptr, last ? val : nullptr);
    else
      hipLaunchKernelGGL(select_kernel<false>, grid, dim3(SEL_THREADS), 0, st, S, ld, label_offset, in, in_stride,
                         p.n[l], p.chunk[l], p.nch[l], k, out, last ? idx : nullptr, last ? val : nullptr);
    TT_CHECK_LAUNCH("select_kernel");
    in = out;
    in_stride = (long)p.nch[l] * k;
  }
  return 0;
}
