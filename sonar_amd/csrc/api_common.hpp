// Shared host-side helpers of the C-ABI translation units (api.hip, decoder_api.hip, ...) and of the files that carve a
// caller's workspace (xsim.hip, mining.hip, align.hip, kmeans.hip, ivf.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <utility>

#include "../../include/sonar_mi355.h"
#include "kernels.hpp"

namespace smi_host {

using namespace smi;

std::string& last_error();

inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  last_error() = buf;
  return code;
}

#define HIP_TRY(expr)                                                                     \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess)                                                                 \
      return smi_host::fail(_e == hipErrorOutOfMemory ? SMI_ERR_OOM : SMI_ERR_HIP,        \
                            "%s failed: %s", #expr, hipGetErrorString(_e));               \
  } while (0)

inline bool have_device() {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) {
    o.p = nullptr;
    o.bytes = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      bytes = o.bytes;
      o.p = nullptr;
      o.bytes = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  hipError_t alloc(size_t n) {
    release();
    if (n == 0) return hipSuccess;
    hipError_t e = hipMalloc(&p, n);
    if (e == hipSuccess) bytes = n;
    return e;
  }
  // grow-only allocation (contents are not preserved)
  hipError_t reserve(size_t n) { return n <= bytes ? hipSuccess : alloc(n); }
  template <typename T>
  T* as() const {
    return (T*)p;
  }
};

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
inline dim3 grid_for(int64_t items, int per_block) { return dim3((unsigned)((items + per_block - 1) / per_block)); }

// A caller-provided workspace, stated once: a layout is a struct over this that take()s its regions in order.  Over a null
// base it only measures (every pointer is null, bytes() is what a *_workspace_bytes function returns); over the caller's
// pointer it carves as well, so the size and the pointers cannot disagree.  A region is `count` T, its size rounded up to
// `align` bytes (so, over a base aligned to `align`, the next region is aligned too); none by default.
class WsLayout {
  char* base_;
  size_t off_ = 0;
 public:
  explicit WsLayout(void* base) : base_((char*)base) {}
  template <typename T>
  T* take(size_t count, size_t align = 1) {
    T* p = base_ ? (T*)(base_ + off_) : nullptr;
    off_ += (size_t)round_up((int64_t)(count * sizeof(T)), (int64_t)align);
    return p;
  }
  size_t bytes() const { return off_; }
};

// A *_workspace_bytes function runs the shape checks of its entry -- the same functions, so it returns 0 exactly where the
// entry refuses on shape -- under this guard: a sizing call leaves smi_last_error() as it was.
struct KeepLastError {
  const std::string text = last_error();
  ~KeepLastError() { last_error() = text; }
};

// The workspace checks of every entry point that takes one; `sizing` is the call that returns `need`.
inline int check_ws(const void* ws, int64_t ws_bytes, size_t need, const char* sizing) {
  if (!ws) return fail(SMI_ERR_INVALID_ARG, "null workspace");
  if ((uintptr_t)ws % 16) return fail(SMI_ERR_INVALID_ARG, "workspace must be 16-byte aligned");
  if (ws_bytes < (int64_t)need)
    return fail(SMI_ERR_INVALID_ARG, "workspace of %lld bytes, %s = %lld", (long long)ws_bytes, sizing, (long long)need);
  return SMI_OK;
}

// The shape checks of the entries over n rows of d fp16 and K buckets of them (`bucket`: "cluster", "list"); row and bucket
// numbers are int32 on the device.  n_name: what the caller calls n, or null where the refusal names nothing (k-means).
inline int check_shape(int64_t n, const char* n_name, int32_t d, int64_t K, const char* bucket) {
  constexpr int64_t kMax = 0x7fffff00LL;
  if (d <= 0 || d % 64) return fail(SMI_ERR_UNSUPPORTED, "d=%d must be a multiple of 64", d);
  if (K < 1) return fail(SMI_ERR_INVALID_ARG, "K=%lld: at least one %s", (long long)K, bucket);
  if (n < 1) return n_name ? fail(SMI_ERR_INVALID_ARG, "%s=%lld: empty input", n_name, (long long)n)
                           : fail(SMI_ERR_INVALID_ARG, "empty input");
  if (n > kMax || K > kMax)
    return fail(SMI_ERR_UNSUPPORTED, "%s=%lld, K=%lld: row and %s numbers must fit int32", n_name ? n_name : "n", (long long)n,
                (long long)K, bucket);
  return SMI_OK;
}

// The shape refusals of the brute-force top-k entries over nx rows against ny: smi_xsim_topk (fit32 false: its pass refuses
// row numbers beyond int32 itself), smi_xsim_topk_page and smi_l2_topk
inline int check_topk_shape(int64_t nx, int64_t ny, int32_t k, int most_k, int32_t d, bool fit32 = true) {
  if (k < 1 || k > most_k) return fail(SMI_ERR_UNSUPPORTED, "k=%d outside [1,%d]", k, most_k);
  if (d <= 0 || d % 64) return fail(SMI_ERR_UNSUPPORTED, "d=%d must be a multiple of 64", d);
  if (nx <= 0 || ny <= 0) return fail(SMI_ERR_INVALID_ARG, "empty input");
  if (fit32 && (nx > 0x7fffff00LL || ny > 0x7fffff00LL))
    return fail(SMI_ERR_UNSUPPORTED, "nx=%lld, ny=%lld: row numbers must fit int32", (long long)nx, (long long)ny);
  return SMI_OK;
}

// Copy a caller tensor into a freshly allocated device buffer as fp16 or fp32;
// `pad_numel` (>= numel) zero-pads the destination.
int upload(const smi_tensor& t, int64_t expect_numel, bool want_f16, DevBuf& dst, const char* name,
           int64_t pad_numel = 0);

// w (row-major [rows][K] fp16 on the device) -> tile-major (common.hpp), in a fresh buffer
inline int to_tile_major(DevBuf& w, int rows, int K) {
  DevBuf t;
  HIP_TRY(t.alloc(w.bytes));
  HIP_TRY(launch_pack_tile_major(w.as<f16>(), t.as<f16>(), rows, K, 0, nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  w = std::move(t);
  return SMI_OK;
}

// Text encoder on the generic-dimension kernels (flex_encoder.hip): configurations the MFMA engines do not tile for
struct FlexEncoder;
bool flex_encoder_wanted(const smi_text_encoder_config& c);
int flex_encoder_create(const smi_text_encoder_config* cfg, const smi_text_encoder_weights* w, FlexEncoder** out);
void flex_encoder_destroy(FlexEncoder* e);
int64_t flex_encoder_bytes(const FlexEncoder* e);
int flex_encoder_forward(FlexEncoder* e, const int64_t* ids, const int32_t* seq_lens, int n, int s, void* out_emb,
                         void* out_encoded, int out_dtype, int32_t* bad_ids_dev, hipStream_t stream);

}  // namespace smi_host
