// The one launcher for kernels that use dynamic LDS: the kernel allowed a size is by construction the kernel launched, and its
// limit is by construction at least the launch's size.
#pragma once
#include <atomic>
#include <mutex>

#include "common.h"
#include "dispatch.h"

namespace arvae {

// Raises K's dynamic-LDS limit to `bytes` unless it is there already.  Called by launch_lds, and by midc_resident_capacity(), which
// asks for K's occupancy before any launch; by nothing else.  The largest size so far is kept per instantiation and process-wide,
// like device_cu_count(): the library assumes one device per process.  The forward and the autograd thread may race here: the
// common path is one relaxed load, a raise is serialised so that a smaller size never lands behind a larger one.
template <auto K> inline void allow_lds(size_t bytes) {
    static std::atomic<size_t> allowed{0};
    if (bytes <= allowed.load(std::memory_order_relaxed)) return;
    static std::mutex raise;
    std::lock_guard<std::mutex> lock(raise);
    if (bytes <= allowed.load(std::memory_order_relaxed)) return;
    // (the result is ignored: check_launch() reports a launch that does not fit)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    allowed.store(bytes, std::memory_order_relaxed);
}

// ARVAE_LAUNCH of kernel K with `lds_bytes` of dynamic LDS
template <auto K, class... A> inline void launch_lds(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, const A &...args) {
    allow_lds<K>(lds_bytes);
    ARVAE_LAUNCH(K, grid, block, lds_bytes, stream, args...);
}

}  // namespace arvae
