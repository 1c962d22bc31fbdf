// Internal (C++) host-side helpers shared by every file that defines entry points of libpfn_hip.so: the error return, the launch with a large dynamic LDS,
// the operand-format predicates and the in-step timing scope.  Nothing here crosses the shared-library boundary; see include/pfn_hip.h for the exported ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "../../include/pfn_hip.h"

namespace pfn {

// Leaves the formatted message for pfn_last_error_string (the calling thread's buffer, pfn_api.hip) and returns `code`.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
#define PFN_TRY(expr)                                                                   \
  do {                                                                                  \
    int rc_ = (expr);                                                                   \
    if (rc_ != PFN_OK) return ::pfn::fail(rc_, "%s failed with %d at %s:%d", #expr, rc_, __FILE__, __LINE__); \
  } while (0)

inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE attribute and setting it costs tens of microseconds of host time, so
// every launcher keeps one of these per kernel: the largest dynamic-LDS size granted so far on each device.  Lock-free; two host
// threads racing on a first use at worst both set the attribute (idempotent) -- neither can launch before it is set.
struct LdsAllowance {
  std::atomic<size_t> granted[16];   // by device ordinal (a node has 8)
  template <typename K> void ensure(K kernel, size_t bytes) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::atomic<size_t>& g = granted[dev & 15];
    if (bytes <= g.load(std::memory_order_acquire)) return;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    size_t cur = g.load(std::memory_order_relaxed);
    while (cur < bytes && !g.compare_exchange_weak(cur, bytes, std::memory_order_release)) {}
  }
};

// A launch with `bytes` of dynamic LDS that raises the kernel's allowance only above the 64 KB a kernel has by default (the BNN step loops, the fold-based
// kernels of the tabular study; other launchers call ensure() unconditionally).  `allow`: the call site's own static, one per kernel instantiation.
template <class... P, class... A>
int launch_lds(void (*kernel)(P...), LdsAllowance& allow, dim3 grid, dim3 block, size_t bytes, hipStream_t s, const A&... args) {
  if (bytes > 64 * 1024) allow.ensure(kernel, bytes);
  kernel<<<grid, block, bytes, s>>>(args...);
  return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
}

// Operand element types (include/pfn_hip.h PFN_PREC_*): two 16-bit formats on the matrix cores at the same rate and bytes, and the exact-f32 parity mode.
inline bool prec_is16(int p) { return p == PFN_PREC_BF16 || p == PFN_PREC_FP16; }
inline int prec_esize(int p) { return prec_is16(p) ? 2 : 4; }

// In-step kernel timing (test / profiling hook pfn_profile_*, pfn_api.hip): an event pair on the launch stream around the launches inside the scope;
// a no-op unless profiling is enabled.
bool prof_enabled();
void* prof_begin(int slot, hipStream_t s);
void prof_end(void* token, int slot, hipStream_t s);
struct ProfScope {
  void* token; int slot; hipStream_t s;
  ProfScope(int slot_, hipStream_t s_) : token(prof_begin(slot_, s_)), slot(slot_), s(s_) {}
  ~ProfScope() { prof_end(token, slot, s); }
  ProfScope(const ProfScope&) = delete;
  ProfScope& operator=(const ProfScope&) = delete;
};

// The "lowbias32" integer finaliser: the hash under the dropout masks (pfn_kernels.h) and the draws of the bar distribution (bar.hip).
__host__ __device__ inline unsigned mix32(unsigned h) {
  h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
  return h;
}

}  // namespace pfn
