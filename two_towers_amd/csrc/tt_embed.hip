// Trainable embedding table: the per-token gradient rows of the layer-0 data gradient summed
// by token id (tt_embed_grad_rows; tt_embed_grad_rows_at puts them at given rows of an otherwise
// zero buffer, which data-parallel ranks then sum), and torch.optim.SparseAdam's update of the
// touched rows with the compute-dtype copy kept in step (tt_sparse_adam_rows). All are HBM-bound.
#include <math.h>

#include <algorithm>

#include "tt_api.h"
#include "tt_common.h"

namespace {

// Sorted positions per workgroup. The work is split by position in the id-sorted list, not
// by segment: token frequencies are Zipf-like, one id may own tens of thousands of rows.
constexpr int CHUNK = 128;
constexpr int UNROLL = 8;  // gathered rows in flight per lane

template <int VEC> struct Vec;
template <> struct Vec<4> {
  typedef float4 T;
  TT_DEV static T zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  TT_DEV static void add(T& a, const T& b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
  TT_DEV static T sel(bool ok, const T& v) { return ok ? v : zero(); }
};
template <> struct Vec<1> {
  typedef float T;
  TT_DEV static T zero() { return 0.f; }
  TT_DEV static void add(T& a, const T& b) { a += b; }
  TT_DEV static T sel(bool ok, const T& v) { return ok ? v : 0.f; }
};

// Largest u in [0, U) with seg_ptr[u] <= p (seg_ptr[0] = 0 <= p < seg_ptr[U] = m).
TT_DEV int segment_of(const int32_t* __restrict__ seg_ptr, int U, long p) {
  int lo = 0, hi = U;
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((long)seg_ptr[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

// Workgroup k owns sorted positions [k CHUNK, (k+1) CHUNK). Lane c owns column group c of
// every row (VEC floats: one 16-byte load per row with VEC 4, so a 1200-byte row is one
// coalesced request of 75 lanes) and walks the positions in order, UNROLL row loads in
// flight, adding them in position order. A segment that lies inside the chunk is written to
// rows[u]; the part of a segment that crosses the chunk's start goes to ws slot 2k, the part
// of one that starts inside and crosses its end to slot 2k+1 (a segment covering the whole
// chunk crosses the start: slot 2k).
// AT: segment u's row is rows[dst[u]] of an [nrows, E] buffer instead of rows[u]; a dst[u]
// outside [0, nrows) drops the segment (tt_embed_grad_rows_at). The sums are the same code.
template <int VEC, bool AT>
TT_DEV void embed_grad_chunk_body(const float* __restrict__ dx, long n, long ldx, const int32_t* __restrict__ perm,
                                  long m, const int32_t* __restrict__ seg_ptr, int U, int E,
                                  const int32_t* __restrict__ dst, int nrows, float* __restrict__ rows,
                                  float* __restrict__ ws) {
  typedef typename Vec<VEC>::T V;
  const long k = blockIdx.x;
  const long p0 = k * CHUNK;
  const long p1 = std::min<long>(m, p0 + CHUNK);
  const int u0 = segment_of(seg_ptr, U, p0);
  const bool head0 = (long)seg_ptr[u0] < p0;
  const int ncol = E / VEC;
  for (int c = threadIdx.x; c < ncol; c += blockDim.x) {
    int u = u0;
    bool head = head0;
    long seg_end = seg_ptr[u + 1];
    V acc = Vec<VEC>::zero();
    long p = p0;
    while (p < p1) {
      const long e = std::min(seg_end, p1);
      for (; p + UNROLL <= e; p += UNROLL) {
        V v[UNROLL];
        bool ok[UNROLL];
#pragma unroll
        for (int i = 0; i < UNROLL; ++i) {
          const long r = perm[p + i];
          ok[i] = (unsigned long)r < (unsigned long)n;  // a row number outside dx adds nothing
          v[i] = *reinterpret_cast<const V*>(dx + (ok[i] ? r : 0) * ldx + (long)c * VEC);
        }
#pragma unroll
        for (int i = 0; i < UNROLL; ++i) Vec<VEC>::add(acc, Vec<VEC>::sel(ok[i], v[i]));
      }
      for (; p < e; ++p) {
        const long r = perm[p];
        const bool ok = (unsigned long)r < (unsigned long)n;
        const V v = *reinterpret_cast<const V*>(dx + (ok ? r : 0) * ldx + (long)c * VEC);
        Vec<VEC>::add(acc, Vec<VEC>::sel(ok, v));
      }
      if (seg_end <= p1) {  // the segment ends in this chunk
        if constexpr (AT) {
          if (head) {
            *reinterpret_cast<V*>(ws + (2 * k) * (long)E + (long)c * VEC) = acc;
          } else {
            const int r = dst[u];
            if ((unsigned)r < (unsigned)nrows) *reinterpret_cast<V*>(rows + (long)r * E + (long)c * VEC) = acc;
          }
        } else {
          float* out = head ? ws + (2 * k) * (long)E : rows + (long)u * E;
          *reinterpret_cast<V*>(out + (long)c * VEC) = acc;
        }
        head = false;
        acc = Vec<VEC>::zero();
        ++u;
        if (u >= U) break;  // p = m = seg_ptr[U] (a seg_ptr that ends short of m stops here too)
        seg_end = seg_ptr[u + 1];
      } else {  // the chunk ends inside the segment
        *reinterpret_cast<V*>(ws + (2 * k + (head ? 0 : 1)) * (long)E + (long)c * VEC) = acc;
      }
    }
  }
}

template <int VEC>
__global__ __launch_bounds__(256) void embed_grad_chunk_kernel(const float* __restrict__ dx, long n, long ldx,
                                                               const int32_t* __restrict__ perm, long m,
                                                               const int32_t* __restrict__ seg_ptr, int U, int E,
                                                               float* __restrict__ rows, float* __restrict__ ws) {
  embed_grad_chunk_body<VEC, false>(dx, n, ldx, perm, m, seg_ptr, U, E, nullptr, 0, rows, ws);
}

// Rows of the [nrows, E] buffer per workgroup of tt_embed_grad_rows_at's zero pass.
constexpr int ZROWS = 64;

// Workgroup z owns rows [z ZROWS, (z+1) ZROWS) and stores +0 to those no dst entry names: one
// lower bound in dst (ascending), then a walk along it; a run of unnamed rows is one contiguous
// range, stored by all threads. The named rows are left to the workgroups that sum them, so no
// element is written twice. Whatever dst holds, the stores stay inside the workgroup's rows.
template <int VEC>
TT_DEV void zero_unnamed_rows(const int32_t* __restrict__ dst, int U, int nrows, int E, float* __restrict__ rows,
                              long z) {
  typedef typename Vec<VEC>::T V;
  const long r0 = z * ZROWS;
  const long r1 = std::min<long>(nrows, r0 + ZROWS);
  int j = 0, hi = U;  // first j with dst[j] >= r0
  while (j < hi) {
    const int mid = j + ((hi - j) >> 1);
    if ((long)dst[mid] < r0) j = mid + 1; else hi = mid;
  }
  for (long r = r0; r < r1; ++j) {
    long named = r1;  // the next named row, or the end
    if (j < U) {
      const long d = dst[j];
      named = d < r ? r : (d < r1 ? d : r1);
    }
    const long b = named * E / VEC;
    for (long i = r * E / VEC + threadIdx.x; i < b; i += blockDim.x) reinterpret_cast<V*>(rows)[i] = Vec<VEC>::zero();
    r = named + 1;
  }
}

// tt_embed_grad_rows_at's first launch: workgroups [0, nchunks) are embed_grad_chunk_kernel's with
// the row of segment u at dst[u], the ones after them run the zero pass beside the gathers.
template <int VEC>
__global__ __launch_bounds__(256) void embed_grad_chunk_at_kernel(const float* __restrict__ dx, long n, long ldx,
                                                                  const int32_t* __restrict__ perm, long m,
                                                                  const int32_t* __restrict__ seg_ptr, int U, int E,
                                                                  const int32_t* __restrict__ dst, int nrows,
                                                                  long nchunks, float* __restrict__ rows,
                                                                  float* __restrict__ ws) {
  if ((long)blockIdx.x >= nchunks) {
    zero_unnamed_rows<VEC>(dst, U, nrows, E, rows, (long)blockIdx.x - nchunks);
    return;
  }
  embed_grad_chunk_body<VEC, true>(dx, n, ldx, perm, m, seg_ptr, U, E, dst, nrows, rows, ws);
}

// Workgroup b - 1 looks at chunk boundary b (position b CHUNK). The segment u holding that
// position crosses it if it starts before it; the workgroup of the first boundary a segment
// crosses adds the segment's partials in chunk order: slot 2 k0 + 1 of the chunk it starts
// in, then slot 2k of every later chunk it reaches. AT as embed_grad_chunk_body.
template <int VEC, bool AT>
TT_DEV void embed_grad_cross_body(long m, const int32_t* __restrict__ seg_ptr, int U, int E,
                                  const int32_t* __restrict__ dst, int nrows, float* __restrict__ rows,
                                  const float* __restrict__ ws) {
  typedef typename Vec<VEC>::T V;
  const long b = (long)blockIdx.x + 1;
  const long p = b * CHUNK;
  const int u = segment_of(seg_ptr, U, p);
  const long s = seg_ptr[u];
  if (s >= p || s < p - CHUNK) return;  // no crossing here, or an earlier boundary's workgroup has it
  const long k0 = b - 1;
  const long k1 = std::min<long>((long)seg_ptr[u + 1] - 1, m - 1) / CHUNK;  // never past the last chunk's slots
  const int ncol = E / VEC;
  for (int c = threadIdx.x; c < ncol; c += blockDim.x) {
    V acc = *reinterpret_cast<const V*>(ws + (2 * k0 + 1) * (long)E + (long)c * VEC);
    long k = k0 + 1;
    for (; k + UNROLL <= k1 + 1; k += UNROLL) {
      V v[UNROLL];
#pragma unroll
      for (int i = 0; i < UNROLL; ++i) v[i] = *reinterpret_cast<const V*>(ws + (2 * (k + i)) * (long)E + (long)c * VEC);
#pragma unroll
      for (int i = 0; i < UNROLL; ++i) Vec<VEC>::add(acc, v[i]);
    }
    for (; k <= k1; ++k) Vec<VEC>::add(acc, *reinterpret_cast<const V*>(ws + (2 * k) * (long)E + (long)c * VEC));
    if constexpr (AT) {
      const int r = dst[u];
      if ((unsigned)r < (unsigned)nrows) *reinterpret_cast<V*>(rows + (long)r * E + (long)c * VEC) = acc;
    } else {
      *reinterpret_cast<V*>(rows + (long)u * E + (long)c * VEC) = acc;
    }
  }
}

template <int VEC>
__global__ __launch_bounds__(256) void embed_grad_cross_kernel(long m, const int32_t* __restrict__ seg_ptr, int U,
                                                               int E, float* __restrict__ rows,
                                                               const float* __restrict__ ws) {
  embed_grad_cross_body<VEC, false>(m, seg_ptr, U, E, nullptr, 0, rows, ws);
}

template <int VEC>
__global__ __launch_bounds__(256) void embed_grad_cross_at_kernel(long m, const int32_t* __restrict__ seg_ptr, int U,
                                                                  int E, const int32_t* __restrict__ dst, int nrows,
                                                                  float* __restrict__ rows,
                                                                  const float* __restrict__ ws) {
  embed_grad_cross_body<VEC, true>(m, seg_ptr, U, E, dst, nrows, rows, ws);
}

inline int block_for(int ncol) { return std::min(256, std::max(64, (ncol + 63) / 64 * 64)); }

// ------------------------------------------------------------------ sparse Adam
struct SparseAdamArgs {
  float* w;
  float* m;
  float* v;
  void* copy;  // [V, ep] compute-dtype copy of w, or null
  const float* g;
  const int32_t* ids;
  const int* skip;
  long vocab, U;
  int E, ep;
  float omb1, omb2, eps, neg_step_size;
};

// torch.optim._functional.sparse_adam on the rows named by ids (values fp32 [U, E]):
//   dm = (g - m) * (1-b1); m += dm; numer = dm + m_old
//   dv = (g*g - v) * (1-b2); v += dv; denom = sqrt(dv + v_old) + eps
//   w += -step_size * (numer / denom),  step_size = lr * sqrt(1-b2^step) / (1-b1^step)
// One wave per row; the rows of ids not in the list are neither read nor written.
template <int VEC, bool BF16>
__global__ __launch_bounds__(256) void sparse_adam_kernel(SparseAdamArgs a) {
  if (a.skip && *a.skip != 0) return;  // an invalid forward fed this step
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.U) return;
  const long u = a.ids[i];
  if ((unsigned long)u >= (unsigned long)a.vocab) return;
  const int lane = threadIdx.x & 63;
  const float* g = a.g + i * (long)a.E;
  float* w = a.w + u * (long)a.E;
  float* m = a.m + u * (long)a.E;
  float* v = a.v + u * (long)a.E;
  for (int c = lane * VEC; c < a.E; c += 64 * VEC) {
    float gv[VEC], wv[VEC], mv[VEC], vv[VEC];
    if constexpr (VEC == 4) {
      const float4 g4 = *reinterpret_cast<const float4*>(g + c), w4 = *reinterpret_cast<const float4*>(w + c);
      const float4 m4 = *reinterpret_cast<const float4*>(m + c), v4 = *reinterpret_cast<const float4*>(v + c);
      gv[0] = g4.x; gv[1] = g4.y; gv[2] = g4.z; gv[3] = g4.w;
      wv[0] = w4.x; wv[1] = w4.y; wv[2] = w4.z; wv[3] = w4.w;
      mv[0] = m4.x; mv[1] = m4.y; mv[2] = m4.z; mv[3] = m4.w;
      vv[0] = v4.x; vv[1] = v4.y; vv[2] = v4.z; vv[3] = v4.w;
    } else {
      gv[0] = g[c]; wv[0] = w[c]; mv[0] = m[c]; vv[0] = v[c];
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const float dm = (gv[j] - mv[j]) * a.omb1;
      const float dv = (gv[j] * gv[j] - vv[j]) * a.omb2;
      const float numer = dm + mv[j];
      const float denom = sqrtf(dv + vv[j]) + a.eps;
      mv[j] = mv[j] + dm;
      vv[j] = vv[j] + dv;
      wv[j] = wv[j] + a.neg_step_size * (numer / denom);
    }
    if constexpr (VEC == 4) {
      *reinterpret_cast<float4*>(m + c) = make_float4(mv[0], mv[1], mv[2], mv[3]);
      *reinterpret_cast<float4*>(v + c) = make_float4(vv[0], vv[1], vv[2], vv[3]);
      *reinterpret_cast<float4*>(w + c) = make_float4(wv[0], wv[1], wv[2], wv[3]);
    } else {
      m[c] = mv[0]; v[c] = vv[0]; w[c] = wv[0];
    }
    if (a.copy) {
      if constexpr (BF16) {
        bf16_t* q = static_cast<bf16_t*>(a.copy) + u * (long)a.ep + c;
        if constexpr (VEC == 4) {
          *reinterpret_cast<uint2*>(q) = make_uint2((uint32_t)f2bf(wv[0]) | ((uint32_t)f2bf(wv[1]) << 16),
                                                    (uint32_t)f2bf(wv[2]) | ((uint32_t)f2bf(wv[3]) << 16));
        } else {
          q[0] = f2bf(wv[0]);
        }
      } else {
        float* q = static_cast<float*>(a.copy) + u * (long)a.ep + c;
        if constexpr (VEC == 4) {
          *reinterpret_cast<float4*>(q) = make_float4(wv[0], wv[1], wv[2], wv[3]);
        } else {
          q[0] = wv[0];
        }
      }
    }
  }
}

}  // namespace

extern "C" int tt_embed_grad_chunk(void) { return CHUNK; }

extern "C" long tt_embed_grad_ws_size(long m, int e) {
  if (m <= 0 || e <= 0) return 256;
  return std::max<long>(256, (long)tt_ceil_div(m, CHUNK) * 2 * e * (long)sizeof(float));
}

extern "C" int tt_embed_grad_rows(const float* dx, long n, long ldx, const int32_t* perm, long m,
                                  const int32_t* seg_ptr, long nseg, int e, float* rows, void* ws, void* stream) {
  TT_CHECK_ARG(n >= 0 && m >= 0 && nseg >= 0 && e >= 1, "tt_embed_grad_rows: bad sizes (n %ld m %ld U %ld E %d)", n, m,
               nseg, e);
  TT_CHECK_ARG(n < (1L << 31) && m < (1L << 31) && nseg < (1L << 31),
               "tt_embed_grad_rows: row numbers and positions are int32");
  TT_CHECK_ARG(nseg <= m, "tt_embed_grad_rows: %ld segments over %ld positions", nseg, m);
  if (nseg == 0 || m == 0 || n == 0) return 0;
  TT_CHECK_ARG(ldx >= e, "tt_embed_grad_rows: ldx %ld < E %d", ldx, e);
  TT_CHECK_ARG(dx && perm && seg_ptr && rows && ws, "tt_embed_grad_rows: null operand");
  const long nchunks = tt_ceil_div(m, CHUNK);
  hipStream_t st = (hipStream_t)stream;
  const bool vec = e % 4 == 0 && ldx % 4 == 0 && ((uintptr_t)dx | (uintptr_t)rows | (uintptr_t)ws) % 16 == 0;
  const int nu = (int)nseg;
  float* w = static_cast<float*>(ws);
  if (vec) {
    const int bs = block_for(e / 4);
    hipLaunchKernelGGL(embed_grad_chunk_kernel<4>, dim3((unsigned)nchunks), dim3(bs), 0, st, dx, n, ldx, perm, m, seg_ptr,
                       nu, e, rows, w);
    TT_CHECK_LAUNCH("embed_grad_chunk_kernel");
    if (nchunks > 1) {
      hipLaunchKernelGGL(embed_grad_cross_kernel<4>, dim3((unsigned)(nchunks - 1)), dim3(bs), 0, st, m, seg_ptr, nu, e,
                         rows, w);
      TT_CHECK_LAUNCH("embed_grad_cross_kernel");
    }
  } else {
    const int bs = block_for(e);
    hipLaunchKernelGGL(embed_grad_chunk_kernel<1>, dim3((unsigned)nchunks), dim3(bs), 0, st, dx, n, ldx, perm, m, seg_ptr,
                       nu, e, rows, w);
    TT_CHECK_LAUNCH("embed_grad_chunk_kernel");
    if (nchunks > 1) {
      hipLaunchKernelGGL(embed_grad_cross_kernel<1>, dim3((unsigned)(nchunks - 1)), dim3(bs), 0, st, m, seg_ptr, nu, e,
                         rows, w);
      TT_CHECK_LAUNCH("embed_grad_cross_kernel");
    }
  }
  return 0;
}

extern "C" int tt_embed_grad_rows_at(const float* dx, long n, long ldx, const int32_t* perm, long m,
                                     const int32_t* seg_ptr, long nseg, const int32_t* dst, long nrows, int e,
                                     float* rows, void* ws, void* stream) {
  TT_CHECK_ARG(n >= 0 && m >= 0 && nseg >= 0 && nrows >= 0 && e >= 1,
               "tt_embed_grad_rows_at: bad sizes (n %ld m %ld U %ld rows %ld E %d)", n, m, nseg, nrows, e);
  TT_CHECK_ARG(n < (1L << 31) && m < (1L << 31) && nseg < (1L << 31) && nrows < (1L << 31),
               "tt_embed_grad_rows_at: row numbers and positions are int32");
  TT_CHECK_ARG(nseg <= m, "tt_embed_grad_rows_at: %ld segments over %ld positions", nseg, m);
  TT_CHECK_ARG(nseg <= nrows, "tt_embed_grad_rows_at: %ld segments for %ld rows", nseg, nrows);
  if (nrows == 0) return 0;
  TT_CHECK_ARG(rows, "tt_embed_grad_rows_at: null operand");
  // nothing to sum (an out-of-range perm entry adds nothing, so n = 0 sums to +0 as well):
  // the zero pass alone writes every row
  const bool sums = nseg > 0 && m > 0 && n > 0;
  if (sums) {
    TT_CHECK_ARG(ldx >= e, "tt_embed_grad_rows_at: ldx %ld < E %d", ldx, e);
    TT_CHECK_ARG(dx && perm && seg_ptr && dst && ws, "tt_embed_grad_rows_at: null operand");
  }
  const long nchunks = sums ? tt_ceil_div(m, CHUNK) : 0;
  const long nzero = tt_ceil_div(nrows, ZROWS);
  hipStream_t st = (hipStream_t)stream;
  const bool vec = e % 4 == 0 && (!sums || (ldx % 4 == 0 && ((uintptr_t)dx | (uintptr_t)ws) % 16 == 0)) &&
                   (uintptr_t)rows % 16 == 0;
  const int nu = sums ? (int)nseg : 0;
  const int nr = (int)nrows;
  float* w = static_cast<float*>(ws);
  if (vec) {
    const int bs = block_for(e / 4);
    hipLaunchKernelGGL(embed_grad_chunk_at_kernel<4>, dim3((unsigned)(nchunks + nzero)), dim3(bs), 0, st, dx, n, ldx,
                       perm, m, seg_ptr, nu, e, dst, nr, nchunks, rows, w);
    TT_CHECK_LAUNCH("embed_grad_chunk_at_kernel");
    if (nchunks > 1) {
      hipLaunchKernelGGL(embed_grad_cross_at_kernel<4>, dim3((unsigned)(nchunks - 1)), dim3(bs), 0, st, m, seg_ptr, nu,
                         e, dst, nr, rows, w);
      TT_CHECK_LAUNCH("embed_grad_cross_at_kernel");
    }
  } else {
    const int bs = block_for(e);
    hipLaunchKernelGGL(embed_grad_chunk_at_kernel<1>, dim3((unsigned)(nchunks + nzero)), dim3(bs), 0, st, dx, n, ldx,
                       perm, m, seg_ptr, nu, e, dst, nr, nchunks, rows, w);
    TT_CHECK_LAUNCH("embed_grad_chunk_at_kernel");
    if (nchunks > 1) {
      hipLaunchKernelGGL(embed_grad_cross_at_kernel<1>, dim3((unsigned)(nchunks - 1)), dim3(bs), 0, st, m, seg_ptr, nu,
                         e, dst, nr, rows, w);
      TT_CHECK_LAUNCH("embed_grad_cross_at_kernel");
    }
  }
  return 0;
}

extern "C" int tt_sparse_adam_rows(float* weight, float* exp_avg, float* exp_avg_sq, long vocab, int e,
                                   const int32_t* ids, const float* rows, long nrows, int copy_dtype, void* copy,
                                   int ep, float lr, float beta1, float beta2, float eps, int step,
                                   const int32_t* skip, void* stream) {
  TT_CHECK_ARG(vocab >= 0 && e >= 1 && nrows >= 0, "tt_sparse_adam_rows: bad sizes (V %ld E %d U %ld)", vocab, e, nrows);
  TT_CHECK_ARG(step >= 1, "tt_sparse_adam_rows: step must be >= 1");
  TT_CHECK_ARG(copy == nullptr || copy_dtype == TT_DT_F32 || copy_dtype == TT_DT_BF16,
               "tt_sparse_adam_rows: bad copy dtype %d", copy_dtype);
  TT_CHECK_ARG(copy == nullptr || ep >= e, "tt_sparse_adam_rows: copy has %d columns < E %d", ep, e);
  TT_CHECK_ARG((nrows + 3) / 4 < (1L << 31), "tt_sparse_adam_rows: too many rows");
  if (nrows == 0 || vocab == 0) return 0;
  TT_CHECK_ARG(weight && exp_avg && exp_avg_sq && ids && rows, "tt_sparse_adam_rows: null operand");
  SparseAdamArgs a{};
  a.w = weight; a.m = exp_avg; a.v = exp_avg_sq; a.copy = copy; a.g = rows; a.ids = ids; a.skip = skip;
  a.vocab = vocab; a.U = nrows; a.E = e; a.ep = ep;
  a.omb1 = (float)(1.0 - (double)beta1);
  a.omb2 = (float)(1.0 - (double)beta2);
  a.eps = eps;
  const double bc1 = 1.0 - pow((double)beta1, step);
  const double bc2 = 1.0 - pow((double)beta2, step);
  a.neg_step_size = (float)(-((double)lr * sqrt(bc2) / bc1));
  const bool bf = copy != nullptr && copy_dtype == TT_DT_BF16;
  const int csz = bf ? 2 : 4;
  const bool vec = e % 4 == 0 &&
                   ((uintptr_t)weight | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)rows) % 16 == 0 &&
                   (copy == nullptr || ((uintptr_t)copy % 16 == 0 && ((long)ep * csz) % 16 == 0));
  const dim3 grid((unsigned)((nrows + 3) / 4));
  hipStream_t st = (hipStream_t)stream;
  if (vec) {
    if (bf) hipLaunchKernelGGL((sparse_adam_kernel<4, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((sparse_adam_kernel<4, false>), grid, dim3(256), 0, st, a);
  } else {
    if (bf) hipLaunchKernelGGL((sparse_adam_kernel<1, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((sparse_adam_kernel<1, false>), grid, dim3(256), 0, st, a);
  }
  TT_CHECK_LAUNCH("sparse_adam_kernel");
  return 0;
}
