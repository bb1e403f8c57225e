// Int8 document index (serving search over one byte per component) and the exact rescoring
// of a shortlist.
//
//   tt_quantize_rows_i8: symmetric per-row codes, one wave per row, one pass.
//   tt_search_topk_i8:   score(i, j) = ((float)dot_ij * ds[j]) * qs[i], dot_ij the exact int32
//     dot product of two code rows; three forms that share the top-k machinery of
//     tt_search_topk (tt_topk.h, tt_topk_rows) and return the same bits:
//       k <= 16, few queries (use_scan): search_scan_i8_kernel, a fused scan: 8 lanes share a row
//         (whole 128-byte lines per load), v_dot4_i32_i8 against query codes staged in LDS,
//         per-lane sorted lists, wave_topk, then topk_merge_kernel. No score matrix.
//       k <= 16, more queries: score_i8_kernel (v_mfma_i32_32x32x32_i8) writes the fp32 score
//         block, then topk_split_kernel and topk_merge_kernel.
//       k > 16: the same score block, then tt_topk_rows.
//   tt_gather_scores:    out[i][r] = qn[i] . dn[cand[i][r]], one wave per (query, candidate).
// Ordering everywhere: value descending, ties towards the lower document index.
#include <cfloat>
#include <climits>

#include "tt_api.h"
#include "tt_common.h"
#include "tt_topk.h"

namespace {

using ttk::SK_MAX;
using ttk::insert;
using ttk::wave_topk;

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int I8_HMAX = 1024;     // |dot| <= 127^2 * 1024 < 2^24: (float)dot is exact
constexpr int SCAN_QMAX = 64;     // most queries the scan takes (option search_i8_qb > 0)
constexpr int WAVE_DOCS = 256;    // documents per scan wave
constexpr int BLK_DOCS = 4 * WAVE_DOCS;
constexpr int ROW_LANES = 8;      // scan lanes per document row: 8 x 16 B = one 128-byte line
constexpr int SCORE_QROWS = 256;  // queries per score_i8_kernel workgroup (8 tiles of 32)

// ------------------------------------------------------------------ quantisation
// One wave per row, lane l holds columns 16 l .. 16 l + 15 (cols <= 1024).
__global__ __launch_bounds__(256) void quantize_rows_i8_kernel(const float* __restrict__ x, long rows, int cols,
                                                               long ld, int8_t* __restrict__ codes,
                                                               float* __restrict__ scale) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int c = lane * 16;
  const bool on = c < cols;
  float a[8], b[8];
  if (on) {
    ld8(x + row * ld + c, a);
    ld8(x + row * ld + c + 8, b);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = b[e] = 0.f;
  }
  float m = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) m = fmaxf(m, fmaxf(fabsf(a[e]), fabsf(b[e])));
  const float amax = wave_max(m);
  const float inv = amax > 0.f ? 127.0f / amax : 0.f;  // IEEE division; a zero row codes to zeros
  if (on) {
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      w[i] = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v = i < 2 ? a[4 * i + e] : b[4 * (i - 2) + e];
        int q = (int)rintf(v * inv);  // round half to even
        q = q < -127 ? -127 : (q > 127 ? 127 : q);
        w[i] |= ((uint32_t)q & 0xFFu) << (8 * e);
      }
    }
    *reinterpret_cast<uint4*>(codes + row * cols + c) = make_uint4(w[0], w[1], w[2], w[3]);
  }
  if (lane == 0) scale[row] = amax / 127.0f;
}

// ------------------------------------------------------------------ fused scan
TT_DEV float i8_score(int dot, float sd, float sq) { return ((float)dot * sd) * sq; }

// Sum over the 8 lanes of a row group (lanes 8 j .. 8 j + 7), left in every one of them.
TT_DEV int row_group_sum(int v) {
  v += __builtin_amdgcn_mov_dpp(v, 0xB1 /* quad_perm [1,0,3,2] */, 0xF, 0xF, false);
  v += __builtin_amdgcn_mov_dpp(v, 0x4E /* quad_perm [2,3,0,1] */, 0xF, 0xF, false);
  v += __builtin_amdgcn_mov_dpp(v, 0x141 /* row_half_mirror */, 0xF, 0xF, false);
  return v;
}

// QB queries per workgroup pass over 1024 documents, 256 per wave. ROW_LANES = 8 lanes share
// a document row: one load instruction reads 8 rows x 128 contiguous bytes, so every cache
// line is fetched once and used whole (a lane per row touches 64 lines per load and leaves
// 7/8 of each for later iterations, far more lines than the L1 holds). Lane l takes the
// 16-byte groups (l & 7) + 8 i of row l >> 3; its partial dot products are summed over the row
// group with DPP adds (integers: any order gives the same sum). The query codes are then no
// longer uniform across the wave (8 distinct groups per load), so they are staged in LDS once
// per workgroup instead of coming through scalar loads. A last group with fewer than QB
// queries stages its last query again in the spare slots and leaves them out of the lists.
// NIT: 128-byte steps per row held in registers (h <= 128 NIT). The next 8 rows' codes are
// loaded before the current ones are scored, so two row groups of loads are in flight per wave.
template <int KM, int QB, int NIT>
__global__ __launch_bounds__(256, (KM * QB <= 16 && NIT <= 4 ? 4 : 2)) void search_scan_i8_kernel(
    const int8_t* __restrict__ qc, const float* __restrict__ qs, long Q, const int8_t* __restrict__ dc,
    const float* __restrict__ ds, long N, int h, int k, float* __restrict__ cv, int* __restrict__ ci) {
  __shared__ i32x4 qlds[QB * NIT * ROW_LANES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cl = lane & (ROW_LANES - 1), rs = lane / ROW_LANES;
  const long q0 = (long)blockIdx.y * QB;
  const int nq = (int)(Q - q0 < QB ? Q - q0 : QB);
  const long nslots = (long)gridDim.x * 4;
  const long slot = (long)blockIdx.x * 4 + wave;
  const int nc = h >> 4;
  for (int t = threadIdx.x; t < QB * nc; t += 256) {
    const int q = t / nc, c = t - q * nc;
    qlds[t] = *reinterpret_cast<const i32x4*>(qc + (q0 + (q < nq ? q : nq - 1)) * h + 16 * c);
  }
  __syncthreads();
  float lv[QB][KM];
  int li[QB][KM];
#pragma unroll
  for (int q = 0; q < QB; ++q) ttk::init<KM>(lv[q], li[q]);
  const i32x4 zero = {0, 0, 0, 0};
  const long wbase = (long)blockIdx.x * BLK_DOCS + wave * WAVE_DOCS;
  const long left = N - wbase;
  const int ng = left <= 0 ? 0 : (left >= WAVE_DOCS ? WAVE_DOCS / 8 : (int)((left + 7) / 8));
  auto load_rows = [&](int g, i32x4(&x)[NIT]) {  // row 8 g + rs of the wave; past N or h: zero codes
    const long d = wbase + 8 * g + rs;
    const bool don = g < ng && d < N;
    const i32x4* row = reinterpret_cast<const i32x4*>(dc + (don ? d : 0) * h);
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int c = ROW_LANES * i + cl;
      x[i] = don && c < nc ? row[c] : zero;
    }
  };
  i32x4 x[NIT], xn[NIT];
  load_rows(0, x);
  for (int g = 0; g < ng; ++g) {
    load_rows(g + 1, xn);
    int acc[QB];
#pragma unroll
    for (int q = 0; q < QB; ++q) acc[q] = 0;
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      if (ROW_LANES * i < nc) {
        const int c = ROW_LANES * i + cl < nc ? ROW_LANES * i + cl : nc - 1;
#pragma unroll
        for (int q = 0; q < QB; ++q) {
          const i32x4 y = qlds[q * nc + c];
          acc[q] = __builtin_amdgcn_sdot4(x[i][0], y[0], acc[q], false);
          acc[q] = __builtin_amdgcn_sdot4(x[i][1], y[1], acc[q], false);
          acc[q] = __builtin_amdgcn_sdot4(x[i][2], y[2], acc[q], false);
          acc[q] = __builtin_amdgcn_sdot4(x[i][3], y[3], acc[q], false);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < QB; ++q) acc[q] = row_group_sum(acc[q]);
    const long d = wbase + 8 * g + rs;
    if (d < N && cl == (g & (ROW_LANES - 1))) {  // the row's 8 lanes take turns keeping its score
      const float sd = ds[d];
#pragma unroll
      for (int q = 0; q < QB; ++q)
        if (q < nq) insert<KM>(lv[q], li[q], k, i8_score(acc[q], sd, qs[q0 + q]), (int)d);
    }
#pragma unroll
    for (int i = 0; i < NIT; ++i) x[i] = xn[i];
  }
#pragma unroll
  for (int q = 0; q < QB; ++q) {
    if (q < nq) {
      const long o = ((q0 + q) * nslots + slot) * k;
      wave_topk<KM>(lv[q], li[q], k, cv + o, ci + o);
    }
  }
}

// ------------------------------------------------------------------ score block
// v_mfma_i32_32x32x32_i8. One wave per 32 documents: their codes stay in registers as the B
// operand (NK steps of K 32), the A operand walks the workgroup's query tiles of 32.
// Fragments come straight from global memory, 16 bytes per lane: lane l holds bytes
// 16 (l >> 5) .. + 15 of K step s of row (l & 31), for A and for B alike, so whatever order
// the instruction takes the 16 bytes of a lane in, both operands agree on it. D register r:
// query row (r & 3) + 8 (r >> 2) + 4 (l >> 5), document column l & 31, so one store
// instruction writes two rows of 32 consecutive scores (whole 128-byte lines where N allows).
// A 16-byte group at or past h reads as zero codes (the K tail).
template <int NK>
__global__ __launch_bounds__(256) void score_i8_kernel(const int8_t* __restrict__ qc, const float* __restrict__ qs,
                                                       long Q, const int8_t* __restrict__ dc,
                                                       const float* __restrict__ ds, long N, int h,
                                                       float* __restrict__ S) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int fr = lane & 31, fh = lane >> 5;
  const long d0 = ((long)blockIdx.x * 4 + wave) * 32;
  if (d0 >= N) return;
  const long d = d0 + fr;
  const bool don = d < N;
  const i32x4 zero = {0, 0, 0, 0};
  i32x4 b[NK];
#pragma unroll
  for (int s = 0; s < NK; ++s) {
    const int kk = 32 * s + 16 * fh;
    b[s] = don && kk < h ? *reinterpret_cast<const i32x4*>(dc + d * h + kk) : zero;
  }
  const float sd = don ? ds[d] : 0.f;
  const long qbeg = (long)blockIdx.y * SCORE_QROWS;
  const long qend = qbeg + SCORE_QROWS < Q ? qbeg + SCORE_QROWS : Q;
  for (long q0 = qbeg; q0 < qend; q0 += 32) {
    const long q = q0 + fr;
    i32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0;
#pragma unroll
    for (int s = 0; s < NK; ++s) {
      if (32 * s < h) {
        const int kk = 32 * s + 16 * fh;
        const i32x4 a = q < Q && kk < h ? *reinterpret_cast<const i32x4*>(qc + q * h + kk) : zero;
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b[s], acc, 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long qq = q0 + (r & 3) + 8 * (r >> 2) + 4 * fh;
      if (qq < Q && don) S[qq * N + d] = i8_score(acc[r], sd, qs[qq]);
    }
  }
}

// ------------------------------------------------------------------ shortlist rescoring
template <typename T>
__global__ __launch_bounds__(256) void gather_scores_kernel(const float* __restrict__ qn, long npairs,
                                                            const T* __restrict__ dn, long N, int h,
                                                            const int32_t* __restrict__ cand, int R,
                                                            float* __restrict__ out) {
  const long p = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (p >= npairs) return;
  const long i = p / R;
  const long j = cand[p];
  float acc = -FLT_MAX;
  if (j >= 0 && j < N) {
    acc = 0.f;
    for (int c = lane * 8; c < h; c += 512) {
      float a[8], b[8];
      ld8(qn + i * h + c, a);
      ld8(dn + j * h + c, b);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc = fmaf(a[e], b[e], acc);
    }
    acc = wave_sum(acc);
  }
  if (lane == 0) out[p] = acc;
}

// ------------------------------------------------------------------ host side
struct I8Ws {
  long cv, ci, cv2, ci2, S, sel, total;
};

// k <= 16: which queries take the fused scan. Measured (profiles/search_i8_ab.txt, N 2^21,
// h 512): one pass of the scan beats the score block (216 vs 326 us at Q 1, k 3), a second pass
// already loses to it (Q 8, k 3: 464 vs 388 us; Q 64: 3372 vs 768 us), so by default the scan
// runs only where one pass holds every query: Q <= 4 (k <= 4) or Q <= 2 (k <= 16). Option
// search_i8_qb > 0 scans up to SCAN_QMAX queries in groups of at most that many, -1 never
// scans; every choice returns the same bits.
inline int scan_group(int k) { return k <= 4 ? 4 : 2; }
inline bool use_scan(long Q, int k) {
  const int o = tt::opt(tt::OPT_SEARCH_I8_QB);
  return o < 0 ? false : Q <= (o > 0 ? SCAN_QMAX : scan_group(k));
}

// The scan's workgroups (1024 documents, four candidate lists each) in G groups of m, the
// last group padded with workgroups past N that write empty lists. One wave merging every
// list of a query is the longest step of a small-Q request on a large index (183 us of 383
// at N 2^21, Q 1, k 3), so the lists are merged in two levels with the same kernel: each
// group's 4 m lists first, then the G results; m ~ sqrt(nblk / 4) balances the two.
struct ScanGeom {
  long nblk, m, G;
};
inline ScanGeom scan_geom(long N) {
  ScanGeom g;
  g.nblk = tt_ceil_div(N, BLK_DOCS);
  if (g.nblk <= 2) { g.m = g.nblk; g.G = 1; return g; }  // one merge
  g.m = 1;
  while (4 * g.m * g.m < g.nblk) ++g.m;
  g.G = tt_ceil_div(g.nblk, g.m);
  return g;
}

// The candidate lists are sized for the scan's padded grid, which also covers the column
// chunks of the split top-k (at most one per 1024 documents), so the size grows with Q.
inline I8Ws i8_ws(long Q, long N, int k) {
  auto al = [](long x) { return (x + 255) & ~255L; };
  I8Ws w{};
  long off = 0;
  if (k > SK_MAX) {
    w.S = off;  off = al(off + Q * N * 4);
    w.sel = off;
    w.total = off + tt_topk_rows_ws_size(Q, N, k);
    return w;
  }
  const ScanGeom g = scan_geom(N);
  const long ncand = g.G * g.m * 4 * k;
  w.cv = off; off = al(off + Q * ncand * 4);
  w.ci = off; off = al(off + Q * ncand * 4);
  w.cv2 = off; off = al(off + Q * g.G * k * 4);
  w.ci2 = off; off = al(off + Q * g.G * k * 4);
  if (!use_scan(Q, k)) { w.S = off; off = al(off + Q * N * 4); }
  w.total = off;
  return w;
}

int i8_scores(const int8_t* qc, const float* qs, long Q, const int8_t* dc, const float* ds, long N, int h, float* S,
              hipStream_t st) {
  const dim3 grid((unsigned)tt_ceil_div(N, 128), (unsigned)tt_ceil_div(Q, SCORE_QROWS));
#define TT_I8_SCORE(NK) \
  hipLaunchKernelGGL((score_i8_kernel<NK>), grid, dim3(256), 0, st, qc, qs, Q, dc, ds, N, h, S)
  if (h <= 64) TT_I8_SCORE(2);
  else if (h <= 128) TT_I8_SCORE(4);
  else if (h <= 256) TT_I8_SCORE(8);
  else if (h <= 512) TT_I8_SCORE(16);
  else TT_I8_SCORE(32);
#undef TT_I8_SCORE
  TT_CHECK_LAUNCH("score_i8_kernel");
  return 0;
}

template <int KM, int QB>
void scan_launch(const int8_t* qc, const float* qs, long Q, const int8_t* dc, const float* ds, long N, int h, int k,
                 float* cv, int* ci, hipStream_t st) {
  const ScanGeom g = scan_geom(N);
  const dim3 grid((unsigned)(g.G * g.m), (unsigned)tt_ceil_div(Q, QB));
#define TT_I8_SCAN(NIT)                                                                                            \
  hipLaunchKernelGGL((search_scan_i8_kernel<KM, QB, NIT>), grid, dim3(256), 0, st, qc, qs, Q, dc, ds, N, h, k, cv, ci)
  if (h <= 128) TT_I8_SCAN(1);
  else if (h <= 256) TT_I8_SCAN(2);
  else if (h <= 512) TT_I8_SCAN(4);
  else TT_I8_SCAN(8);
#undef TT_I8_SCAN
}

// Queries per scan pass: the smallest instantiated group that holds Q, up to the cap
// (option search_i8_qb, else scan_group).
template <int KM>
int i8_launch(const int8_t* qc, const float* qs, long Q, const int8_t* dc, const float* ds, long N, int h, int k,
              int32_t* idx, float* val, char* ws, hipStream_t st) {
  const I8Ws w = i8_ws(Q, N, k);
  float* cv = reinterpret_cast<float*>(ws + w.cv);
  int* ci = reinterpret_cast<int*>(ws + w.ci);
  long ncand;
  const int qb_opt = tt::opt(tt::OPT_SEARCH_I8_QB);
  if (use_scan(Q, k)) {
    const ScanGeom g = scan_geom(N);
    ncand = g.G * g.m * 4 * k;
    constexpr int QB_TOP = KM <= 4 ? 8 : 2, QB_DFLT = KM <= 4 ? 4 : 2;
    int cap = qb_opt;
    cap = cap <= 0 ? QB_DFLT : (cap > QB_TOP ? QB_TOP : cap);
    int qb = 1;
    while (qb < cap && qb < Q) qb *= 2;
    if (qb == 1) scan_launch<KM, 1>(qc, qs, Q, dc, ds, N, h, k, cv, ci, st);
    else if (qb == 2) scan_launch<KM, 2>(qc, qs, Q, dc, ds, N, h, k, cv, ci, st);
    else if (KM <= 4 && qb == 4) scan_launch<KM, (KM <= 4 ? 4 : 2)>(qc, qs, Q, dc, ds, N, h, k, cv, ci, st);
    else scan_launch<KM, QB_TOP>(qc, qs, Q, dc, ds, N, h, k, cv, ci, st);
    TT_CHECK_LAUNCH("search_scan_i8_kernel");
    if (g.G > 1) {  // first level: the 4 m lists of each group, one wave per (query, group)
      float* cv2 = reinterpret_cast<float*>(ws + w.cv2);
      int* ci2 = reinterpret_cast<int*>(ws + w.ci2);
      hipLaunchKernelGGL((ttk::topk_merge_kernel<KM>), dim3((unsigned)tt_ceil_div(Q * g.G, 4)), dim3(256), 0, st, cv, ci,
                         Q * g.G, g.m * 4 * k, k, ci2, cv2);
      TT_CHECK_LAUNCH("topk_merge_kernel");
      cv = cv2;
      ci = ci2;
      ncand = g.G * k;
    }
  } else {
    float* S = reinterpret_cast<float*>(ws + w.S);
    TT_PROPAGATE(i8_scores(qc, qs, Q, dc, ds, N, h, S, st));
    const long chunk = ttk::split_chunk(Q, N), nsp = tt_ceil_div(N, chunk);
    ncand = nsp * k;
    hipLaunchKernelGGL((ttk::topk_split_kernel<KM>), dim3((unsigned)tt_ceil_div(Q, 4), (unsigned)nsp), dim3(256), 0,
                       st, S, Q, N, chunk, -1L, k, cv, ci);
    TT_CHECK_LAUNCH("topk_split_kernel");
  }
  hipLaunchKernelGGL((ttk::topk_merge_kernel<KM>), dim3((unsigned)tt_ceil_div(Q, 4)), dim3(256), 0, st, cv, ci, Q, ncand,
                     k, idx, val);
  TT_CHECK_LAUNCH("topk_merge_kernel");
  return 0;
}

}  // namespace

extern "C" int tt_quantize_rows_i8(const float* x, long rows, int cols, long ld, int8_t* codes, float* scale,
                                   void* stream) {
  TT_CHECK_ARG(cols > 0 && cols % 16 == 0 && cols <= I8_HMAX,
               "tt_quantize_rows_i8: cols=%d must be a multiple of 16 and at most %d", cols, I8_HMAX);
  TT_CHECK_ARG(rows >= 0 && rows <= (long)INT_MAX * 4 && ld >= cols && ld % 4 == 0,
               "tt_quantize_rows_i8: rows=%ld ld=%ld (ld >= cols, ld %% 4 == 0)", rows, ld);
  if (rows == 0) return 0;
  TT_CHECK_ARG(x && codes && scale && ((uintptr_t)x | (uintptr_t)codes) % 16 == 0,
               "tt_quantize_rows_i8: x and codes must be 16-byte aligned");
  hipLaunchKernelGGL(quantize_rows_i8_kernel, dim3((unsigned)tt_ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream,
                     x, rows, cols, ld, codes, scale);
  TT_CHECK_LAUNCH("quantize_rows_i8_kernel");
  return 0;
}

extern "C" long tt_search_i8_ws_size(long Q, long N, int h, int k) {
  (void)h;
  return i8_ws(Q, N, k).total;
}

extern "C" int tt_search_topk_i8(const int8_t* qc, const float* qs, long Q, const int8_t* dc, const float* ds, long N,
                                 int h, int k, int32_t* idx, float* val, void* ws, void* stream) {
  TT_CHECK_ARG(k >= 1 && k <= ttk::SEL_MAX && k <= N, "tt_search_topk_i8: k=%d needs 1 <= k <= min(%d, N=%ld)", k,
               ttk::SEL_MAX, N);
  TT_CHECK_ARG(h > 0 && h % 16 == 0 && h <= I8_HMAX,
               "tt_search_topk_i8: h=%d must be a multiple of 16 and at most %d", h, I8_HMAX);
  TT_CHECK_ARG(N <= INT_MAX && Q >= 0 && Q <= 65535L * 4, "tt_search_topk_i8: N=%ld Q=%ld", N, Q);
  TT_CHECK_ARG(((uintptr_t)dc | (uintptr_t)qc) % 16 == 0, "tt_search_topk_i8: code matrices must be 16-byte aligned");
  if (Q == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  char* ws_c = static_cast<char*>(ws);
  if (k > SK_MAX) {
    const I8Ws w = i8_ws(Q, N, k);
    float* S = reinterpret_cast<float*>(ws_c + w.S);
    TT_PROPAGATE(i8_scores(qc, qs, Q, dc, ds, N, h, S, st));
    return tt_topk_rows(S, Q, N, N, -1L, k, idx, val, ws_c + w.sel, stream);
  }
  if (k <= 4) return i8_launch<4>(qc, qs, Q, dc, ds, N, h, k, idx, val, ws_c, st);
  return i8_launch<SK_MAX>(qc, qs, Q, dc, ds, N, h, k, idx, val, ws_c, st);
}

extern "C" int tt_gather_scores(int dtype, const float* qn, long Q, const void* dn, long N, int h, const int32_t* cand,
                                int R, float* out, void* stream) {
  TT_CHECK_ARG(dtype == TT_DT_F32 || dtype == TT_DT_BF16, "tt_gather_scores: bad dtype");
  TT_CHECK_ARG(h > 0 && h % 8 == 0, "tt_gather_scores: h=%d must be a multiple of 8", h);
  TT_CHECK_ARG(R >= 1 && R <= ttk::SEL_MAX, "tt_gather_scores: R=%d needs 1 <= R <= %d", R, ttk::SEL_MAX);
  TT_CHECK_ARG(N >= 0 && N <= INT_MAX && Q >= 0 && Q <= 65535L * 4, "tt_gather_scores: N=%ld Q=%ld", N, Q);
  TT_CHECK_ARG(((uintptr_t)dn | (uintptr_t)qn) % 16 == 0, "tt_gather_scores: operands must be 16-byte aligned");
  if (Q == 0) return 0;
  const long npairs = Q * R;
  const dim3 grid((unsigned)tt_ceil_div(npairs, 4));
  if (dtype == TT_DT_BF16)
    hipLaunchKernelGGL((gather_scores_kernel<bf16_t>), grid, dim3(256), 0, (hipStream_t)stream, qn, npairs,
                       (const bf16_t*)dn, N, h, cand, R, out);
  else
    hipLaunchKernelGGL((gather_scores_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, qn, npairs,
                       (const float*)dn, N, h, cand, R, out);
  TT_CHECK_LAUNCH("gather_scores_kernel");
  return 0;
}
