// averaging.hpp — the host front end of the averaging operators (spectral_mean.hip,
// spectral_matrix.hip, bispectrum.hip, wavenumber.hip, correlation.hip): the arithmetic on a
// plan that splits a call into frames, groups and chunks, the argument checks every entry
// makes, the shared workspace of per-frame spectra and the launch check. Host code only.
//
// Every check returns SPECENH_OK (0) or a negative error recorded through set_error, so a
// call site reads `if (int rc = check(...)) return rc;`. An entry checks in this order: its
// input pointers, check_call (plan, batch, frame split), strides, its own arguments, outputs;
// batch == 0 then returns SPECENH_OK; the workspace comes last.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "specenh_spectral.h"
#include "runtime.hpp"
#include "stft_plan.hpp"

namespace specenh {

// Real frames transformed side by side by a CSM or bispectrum workgroup: 8 where two buffers
// of S * N/2 complex fit 64 KiB.
inline int slots8_for(int N) { return N <= 1024 ? 8 : 8192 / N; }
// ... by a spectral_mean or correlation workgroup: 256 (512 zero-padded) radix-4 butterflies a
// pass where N allows, at least x and y.
inline int slots_for(int N) { return N >= 1024 ? 2 : 2048 / N; }

// Frames, groups, frames per group, frames that enter a group and chunks (runs of at most
// SPECENH_SPECTRAL_CHUNK frames) per group of an averaging call.
struct FrameSplit {
  long long T, G, glen, Tu, ncg;
};
// Fills *s or returns a negative error; lds_sizes: nperseg must be one the LDS transform has.
inline int frame_split(const specenh_stft_plan* plan, long long length, long long navg,
                       bool lds_sizes, FrameSplit* s) {
  const int N = plan->nperseg;
  if (lds_sizes && (N < 64 || N > 4096 || (N & (N - 1))))
    return set_error(SPECENH_EUNSUPPORTED, "nperseg must be a power of two in [64, 4096]");
  s->T = specenh_stft_frames(length, N, plan->noverlap);
  if (s->T < 0) return (int)s->T;
  s->G = specenh_spectral_groups(s->T, navg);
  if (s->G < 0) return (int)s->G;
  if (s->T > (1ll << 30)) return set_error(SPECENH_EINVAL, "too many frames");
  s->glen = navg >= 1 ? navg : s->T;
  s->Tu = s->G * s->glen;
  s->ncg = (s->glen + SPECENH_SPECTRAL_CHUNK - 1) / SPECENH_SPECTRAL_CHUNK;
  return SPECENH_OK;
}

// What an entry and its *_workspace_bytes function check alike: the plan, the batch, the split.
inline int check_call(const specenh_stft_plan* plan, long long batch, long long length,
                      long long navg, bool lds_sizes, FrameSplit* s) {
  if (!plan) return set_error(SPECENH_EINVAL, "null plan");
  if (batch < 0) return set_error(SPECENH_EINVAL, "batch must be >= 0");
  return frame_split(plan, length, navg, lds_sizes, s);
}

// `what`: the message, "x_stride < length".
inline int check_stride(long long stride, long long length, const char* what) {
  return stride < length ? set_error(SPECENH_EINVAL, what) : SPECENH_OK;
}

// A signal argument of an entry: shot b at p + b * stride; p may be null where the entry lets
// the signal default to the first one.
struct SignalArg {
  const float* p;
  long long stride;
  const char* short_stride;  // check_stride's message
};
inline int check_strides(const SignalArg* in, int n, long long length) {
  for (int v = 0; v < n; ++v)
    if (in[v].p)
      if (int rc = check_stride(in[v].stride, length, in[v].short_stride)) return rc;
  return SPECENH_OK;
}

// The distinct signals of a call: shot b of signal s at p[s] + b * stride[s].
struct FrameSignals {
  const float* p[3];
  long long stride[3];
};
// Fills *sig from in[0 .. n), n <= 3, and returns how many are distinct: two arguments are one
// signal when pointer and stride agree, a null one is in[0]. which[v]: the signal argument v is.
inline int collect_signals(const SignalArg* in, int n, FrameSignals* sig, int* which) {
  int nsig = 0;
  for (int v = 0; v < n; ++v) {
    const SignalArg& a = in[v].p ? in[v] : in[0];
    int found = -1;
    for (int u = 0; u < nsig; ++u)
      if (sig->p[u] == a.p && sig->stride[u] == a.stride) found = u;
    if (found < 0) {
      sig->p[nsig] = a.p;
      sig->stride[nsig] = a.stride;
      found = nsig++;
    }
    which[v] = found;
  }
  return nsig;
}

// A workspace of `bytes` bytes against the `need` of the call.
inline int check_workspace(const void* workspace, size_t bytes, size_t need) {
  if (!workspace) return set_error(SPECENH_EINVAL, "null workspace");
  if (reinterpret_cast<size_t>(workspace) % 16)
    return set_error(SPECENH_EINVAL, "workspace must be 16-byte aligned");
  if (bytes < need) return set_error(SPECENH_EINVAL, "workspace too small");
  return SPECENH_OK;
}

// Bytes of transform_frames' workspace: float2 [batch][nsig][Tu][F].
inline size_t frames_workspace_bytes(const specenh_stft_plan* plan, long long batch,
                                     long long nsig, long long Tu) {
  return (size_t)batch * (size_t)nsig * (size_t)Tu * (size_t)(plan->nperseg / 2 + 1) *
         sizeof(float2);
}
// Detrends, windows and transforms frames [0, Tu) of every signal of every shot, once, into
// `workspace` as float2 [batch][nsig][Tu][F] holding 2 X / sqrt(plan->scale) (defined in
// bispectrum.hip beside its kernel). SPECENH_OK or a negative error.
int transform_frames(const specenh_stft_plan* plan, const FrameSignals& sig, int nsig,
                     long long batch, long long Tu, void* workspace, hipStream_t stream);

// The channel-array form: detrends, windows and transforms frames [0, Tu) of the C channels of
// nb <= 65535 shots, once, into `ws` as float2 [nb][F][Tu][C] holding 2 X (defined in
// spectral_matrix.hip beside its kernel; what specenh_csm and specenh_array_spectrum sum).
// SPECENH_OK or a negative error.
int csm_transform(const specenh_stft_plan* plan, const float* x, long long nb, int C,
                  long long channel_stride, long long batch_stride, long long Tu, float2* ws,
                  hipStream_t stream);

// Spectra the caller holds, [batch][frames][nfreq]: fills *G (groups).
inline int check_spectra(long long batch, long long frames, long long nfreq, long long navg,
                         long long* G) {
  if (batch < 0) return set_error(SPECENH_EINVAL, "batch must be >= 0");
  if (nfreq < 1 || nfreq > 2049) return set_error(SPECENH_EINVAL, "nfreq must be in [1, 2049]");
  if (frames > (1ll << 30)) return set_error(SPECENH_EINVAL, "too many frames");
  *G = specenh_spectral_groups(frames, navg);
  return *G < 0 ? (int)*G : SPECENH_OK;
}

// SPECENH_LAUNCH for a kernel held in a function pointer.
template <class K, class A>
inline void launch(K kernel, dim3 grid, dim3 block, size_t lds, void* stream, const A& args) {
  note_launch(reinterpret_cast<const void*>(kernel));
  hipLaunchKernelGGL(kernel, grid, block, lds, (hipStream_t)stream, args);
}

// After a launch: SPECENH_OK, or SPECENH_EHIP with "<name> launch: <hip string>".
inline int launched(const char* name) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return SPECENH_OK;
  return set_error(SPECENH_EHIP, std::string(name) + " launch: " + hipGetErrorString(e));
}

}  // namespace specenh
