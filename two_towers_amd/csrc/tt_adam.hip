// Multi-tensor Adam / AdamW: one launch updates every parameter of the model; the
// gradient norm over the same tensor lists and the clip_grad_norm_ scaling.
#include <math.h>

#include <algorithm>

#include "tt_api.h"
#include "tt_common.h"

namespace {

constexpr int MAXT = 48;
constexpr int CHUNK = 4096;  // elements per workgroup

struct AdamArgs {
  float* p[MAXT];
  const float* g[MAXT];
  float* m[MAXT];
  float* v[MAXT];
  long start[MAXT + 1];  // prefix sums of sizes
  const int* skip;       // device word: non-zero -> leave every tensor unchanged (or null)
  int nt;
  float b2, omb1, omb2, eps, wd, step_size, bc2_sqrt;
  float decay;  // DECOUPLED: (float)(1 - lr * wd)
};

// Matches torch.optim.adam._single_tensor_adam (foreach=False, capturable=False):
//   exp_avg.lerp_(grad, 1-b1); exp_avg_sq.mul_(b2).addcmul_(grad, grad, value=1-b2)
//   denom = exp_avg_sq.sqrt() / bias_correction2_sqrt + eps
//   param.addcdiv_(exp_avg, denom, value=-lr/bias_correction1)
// DECOUPLED (torch.optim.adamw, single tensor): param.mul_(1 - lr * weight_decay) first,
// then the update above with grad untouched.
template <bool DECOUPLED>
__global__ __launch_bounds__(256) void adam_kernel(AdamArgs a) {
  if (a.skip && *a.skip != 0) return;  // an invalid forward fed this step
  const long e0 = (long)blockIdx.x * CHUNK;
  const long total = a.start[a.nt];
  int t = 0;
  while (t + 1 < a.nt && a.start[t + 1] <= e0) ++t;
  for (long e = e0 + threadIdx.x; e < min(total, e0 + CHUNK); e += 256) {
    while (e >= a.start[t + 1]) ++t;
    const long i = e - a.start[t];
    float g = a.g[t][i];
    float p = a.p[t][i];
    if constexpr (DECOUPLED) {
      p = p * a.decay;
    } else {
      if (a.wd != 0.f) g = g + a.wd * p;
    }
    float m = a.m[t][i];
    float v = a.v[t][i];
    m = m + a.omb1 * (g - m);  // lerp, weight < 0.5 branch
    v = v * a.b2 + a.omb2 * g * g;
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    p = p + (-a.step_size * m) / denom;
    a.m[t][i] = m;
    a.v[t][i] = v;
    a.p[t][i] = p;
  }
}

// ------------------------------------------------------------ gradient norm, clip
struct GradArgs {
  float* g[MAXT];
  long start[MAXT + 1];
  int nt;
};

// sum of one 4096-element chunk: 16 elements per thread in index order, the wave's 64
// sums by a fixed butterfly, the four waves in order
TT_DEV float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(GradArgs a, float* __restrict__ part) {
  __shared__ float red[4];
  const long e0 = (long)blockIdx.x * CHUNK;
  const long total = a.start[a.nt];
  int t = 0;
  while (t + 1 < a.nt && a.start[t + 1] <= e0) ++t;
  float ss = 0.f;
  for (long e = e0 + threadIdx.x; e < min(total, e0 + CHUNK); e += 256) {
    while (e >= a.start[t + 1]) ++t;
    const float g = a.g[t][e - a.start[t]];
    ss += g * g;
  }
  ss = block_sum(ss, red);
  if (threadIdx.x == 0) part[blockIdx.x] = ss;
}

// one workgroup: thread t adds partials t, t + 256, ... in ascending order, then the
// fixed block reduction; sumsq[0] (+)= the total
__global__ __launch_bounds__(256) void grad_sumsq_final_kernel(const float* __restrict__ part, long nparts,
                                                               int accumulate, float* __restrict__ sumsq) {
  __shared__ float red[4];
  float s = 0.f;
  for (long i = threadIdx.x; i < nparts; i += 256) s += part[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) sumsq[0] = accumulate ? sumsq[0] + s : s;
}

// torch.nn.utils.clip_grad_norm_: coef = clamp(max_norm / (total + 1e-6), max=1), g *= coef.
// The comparison keeps a NaN coefficient a NaN (error_if_nonfinite=False propagates it).
__global__ __launch_bounds__(256) void clip_scale_kernel(GradArgs a, const float* __restrict__ sumsq, float max_norm,
                                                         float* __restrict__ total_out) {
  const float total_norm = sqrtf(sumsq[0]);
  const float c = max_norm / (total_norm + 1e-6f);
  const float coef = c > 1.f ? 1.f : c;
  if (total_out && blockIdx.x == 0 && threadIdx.x == 0) total_out[0] = total_norm;
  const long e0 = (long)blockIdx.x * CHUNK;
  const long total = a.start[a.nt];
  int t = 0;
  while (t + 1 < a.nt && a.start[t + 1] <= e0) ++t;
  for (long e = e0 + threadIdx.x; e < min(total, e0 + CHUNK); e += 256) {
    while (e >= a.start[t + 1]) ++t;
    float* p = a.g[t] + (e - a.start[t]);
    *p = *p * coef;
  }
}

inline void grad_args(GradArgs& a, float* const* grads, const long* sizes, int ntensors) {
  a.start[0] = 0;
  for (int i = 0; i < ntensors; ++i) {
    a.g[i] = grads[i];
    a.start[i + 1] = a.start[i] + sizes[i];
  }
  a.nt = ntensors;
}

}  // namespace

extern "C" long tt_grad_norm_ws_size(const long* sizes, int ntensors) {
  long total = 0;
  for (int i = 0; i < ntensors; ++i) total += sizes[i];
  return std::max<long>(256, (long)tt_ceil_div(total, CHUNK) * (long)sizeof(float));
}

extern "C" int tt_grad_norm_multi(const float* const* grads, const long* sizes, int ntensors, int accumulate,
                                  float* sumsq, void* ws, void* stream) {
  TT_CHECK_ARG(ntensors >= 0 && ntensors <= MAXT, "tt_grad_norm_multi: at most %d tensors per call", MAXT);
  TT_CHECK_ARG(sumsq != nullptr, "tt_grad_norm_multi: null sumsq");
  for (int i = 0; i < ntensors; ++i) TT_CHECK_ARG(sizes[i] >= 0, "tt_grad_norm_multi: negative size");
  GradArgs a{};
  grad_args(a, const_cast<float* const*>(reinterpret_cast<const float* const*>(grads)), sizes, ntensors);
  const long total = a.start[ntensors];
  const long nparts = tt_ceil_div(total, CHUNK);
  TT_CHECK_ARG(nparts == 0 || ws != nullptr, "tt_grad_norm_multi: null workspace");
  hipStream_t st = (hipStream_t)stream;
  if (nparts > 0) {
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)nparts), dim3(256), 0, st, a, static_cast<float*>(ws));
    TT_CHECK_LAUNCH("grad_sumsq_kernel");
  }
  hipLaunchKernelGGL(grad_sumsq_final_kernel, dim3(1), dim3(256), 0, st, static_cast<const float*>(ws), nparts,
                     accumulate, sumsq);
  TT_CHECK_LAUNCH("grad_sumsq_final_kernel");
  return 0;
}

extern "C" int tt_clip_scale_multi(float* const* grads, const long* sizes, int ntensors, const float* sumsq,
                                   float max_norm, float* total_norm_out, void* stream) {
  TT_CHECK_ARG(ntensors >= 0 && ntensors <= MAXT, "tt_clip_scale_multi: at most %d tensors per call", MAXT);
  TT_CHECK_ARG(sumsq != nullptr, "tt_clip_scale_multi: null sumsq");
  for (int i = 0; i < ntensors; ++i) TT_CHECK_ARG(sizes[i] >= 0, "tt_clip_scale_multi: negative size");
  GradArgs a{};
  grad_args(a, grads, sizes, ntensors);
  const long total = a.start[ntensors];
  // at least one workgroup, so total_norm_out is written even with nothing to scale
  hipLaunchKernelGGL(clip_scale_kernel, dim3((unsigned)std::max(1, tt_ceil_div(total, CHUNK))), dim3(256), 0,
                     (hipStream_t)stream, a, sumsq, max_norm, total_norm_out);
  TT_CHECK_LAUNCH("clip_scale_kernel");
  return 0;
}

template <bool DECOUPLED>
static int adam_launch(const char* who, float* const* params, const float* const* grads, float* const* exp_avg,
                       float* const* exp_avg_sq, const long* sizes, int ntensors, float lr, float beta1, float beta2,
                       float eps, float weight_decay, int step, const int32_t* skip, void* stream) {
  TT_CHECK_ARG(ntensors >= 0 && ntensors <= MAXT, "%s: at most %d tensors per call", who, MAXT);
  TT_CHECK_ARG(step >= 1, "%s: step must be >= 1", who);
  if (ntensors == 0) return 0;
  AdamArgs a{};
  a.start[0] = 0;
  for (int i = 0; i < ntensors; ++i) {
    a.p[i] = params[i];
    a.g[i] = grads[i];
    a.m[i] = exp_avg[i];
    a.v[i] = exp_avg_sq[i];
    a.start[i + 1] = a.start[i] + sizes[i];
  }
  a.nt = ntensors;
  a.skip = skip;
  a.b2 = beta2; a.omb1 = (float)(1.0 - (double)beta1); a.omb2 = (float)(1.0 - (double)beta2);
  a.eps = eps; a.wd = weight_decay;
  a.decay = (float)(1.0 - (double)lr * (double)weight_decay);
  const double bc1 = 1.0 - pow((double)beta1, step);
  const double bc2 = 1.0 - pow((double)beta2, step);
  a.step_size = (float)(lr / bc1);
  a.bc2_sqrt = (float)sqrt(bc2);
  const long total = a.start[ntensors];
  if (total == 0) return 0;
  hipLaunchKernelGGL(adam_kernel<DECOUPLED>, dim3((unsigned)tt_ceil_div(total, CHUNK)), dim3(256), 0,
                     (hipStream_t)stream, a);
  TT_CHECK_LAUNCH("adam_kernel");
  return 0;
}

extern "C" int tt_adam_multi(float* const* params, const float* const* grads, float* const* exp_avg,
                             float* const* exp_avg_sq, const long* sizes, int ntensors, float lr, float beta1,
                             float beta2, float eps, float weight_decay, int step, const int32_t* skip,
                             void* stream) {
  return adam_launch<false>("tt_adam_multi", params, grads, exp_avg, exp_avg_sq, sizes, ntensors, lr, beta1, beta2, eps,
                            weight_decay, step, skip, stream);
}

extern "C" int tt_adamw_multi(float* const* params, const float* const* grads, float* const* exp_avg,
                              float* const* exp_avg_sq, const long* sizes, int ntensors, float lr, float beta1,
                              float beta2, float eps, float weight_decay, int step, const int32_t* skip,
                              void* stream) {
  return adam_launch<true>("tt_adamw_multi", params, grads, exp_avg, exp_avg_sq, sizes, ntensors, lr, beta1, beta2, eps,
                           weight_decay, step, skip, stream);
}
