// What the host side of a stand-alone operator needs and nothing of the model: the workspace allocator, and the record of one
// call with the three things every entry point does around its kernels.  An operator has ONE carve function per call that
// takes its tensors from a Ws: vsp_*_workspace_bytes is that function's dry pass, the entry point runs it on the caller's
// bytes and refuses what is shorter than the same `cur` -- a size and its run cannot disagree.
#pragma once
#include <cstddef>
#include <cstdint>

#include "model.h"

namespace vsp {

struct T3 {
  float* p = nullptr;
  long bs = 0, cs = 0;
  T3 chan(int c) const { return T3{p ? p + (size_t)c * cs : nullptr, bs, cs}; }
};

// Bump allocator over the caller's workspace; in dry mode it only measures.
struct Ws {
  char* base;
  size_t cap;
  size_t cur = 0;
  bool dry;
  bool overflow = false;
  Ws(void* b, size_t c, bool d) : base((char*)b), cap(c), dry(d) {}
  void* bytes(size_t n) {
    const size_t o = cur;
    cur += (n + 255) / 256 * 256;
    if (dry) return nullptr;
    if (cur > cap) { overflow = true; return nullptr; }
    return base + o;
  }
  float* f(size_t n) { return (float*)bytes(n * sizeof(float)); }
  T3 t3(int B, int C, int T) {
    const long ts = (T + 63) / 64 * 64;
    T3 t;
    t.p = f((size_t)B * C * ts);
    t.cs = ts;
    t.bs = (long)C * ts;
    return t;
  }
};

inline Ws dry_ws() { return Ws(nullptr, 0, true); }

// One call of an operator: who reports, on which stream.
struct Call {
  vsp_ctx* ctx;
  const char* who;
  hipStream_t s;
  // The caller's workspace to carve from: what does not fit comes back as NULL and is refused by need_ws() before any use.
  Ws open(void* workspace, int64_t workspace_bytes) const {
    return Ws(workspace, workspace && workspace_bytes > 0 ? (size_t)workspace_bytes : 0, false);
  }
  int need_ws(const void* workspace, int64_t workspace_bytes, size_t need) const {
    if (!workspace || workspace_bytes < (int64_t)need)
      return ctx->fail(VSP_ERR_WORKSPACE, "%s: the workspace needs %lld bytes", who, (long long)need);
    return VSP_OK;
  }
  // Host memory to the workspace.  The memory is PAGEABLE -- the caller's array, a local vector, a table whose lock is dropped
  // right after the call -- and the upload rests on the runtime reading such memory into its own staging buffer before
  // hipMemcpyAsync returns (as api_frame.hip does for the noise seeds and the row controls).  That blocks the host for the
  // copy, and it is why these calls cannot be captured into a graph.
  int upload(void* dst, const void* src, size_t bytes, const char* what = "rows") const {
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "%s (%s): %s", who, what, hipGetErrorString(e));
    return VSP_OK;
  }
  // After hipLaunchKernelGGL: `what` names the kernel (or the launches, where several share one check).
  int launched(const char* what) const {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return VSP_OK;
  }
};

}  // namespace vsp
