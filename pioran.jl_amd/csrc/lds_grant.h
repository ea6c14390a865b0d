// Raising a kernel's dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize): every launcher that needs more than the default asks here,
// right before its launch.  The attribute belongs to (kernel, device), and one process may drive several devices from several threads
// (pioran_farm_*), so what has been granted is remembered process-wide, per device, behind a mutex — not per thread (the farm starts fresh threads
// on every call), and not in a static of the launcher.  Host code only; header-only so that a probe which includes one kernel source links alone.
#pragma once
#include "common.h"

#include <initializer_list>
#include <mutex>
#include <vector>

struct LdsGrant {
    const void* kernel;
    size_t bytes;
};

// PIORAN_OK: every kernel of the list may be launched with its `bytes` of dynamic LDS on the calling thread's current device (any ordinal); a launch
// that runs two such kernels asks for both at once (an entry without a kernel is passed over).  Where each was granted at least as much before, the
// call costs one hipGetDevice, an uncontended lock and a look through a short vector; no other runtime call.  PIORAN_ERR_HIP: the runtime refuses
// one — the sticky error is cleared and the refusal remembered for the life of the process, so that a launcher with a fallback (dense.hip's tile
// build) does not ask again on every call.  A launcher without one inherits that: after a refusal, every later launch of that kernel at that size
// or above fails with PIORAN_ERR_HIP without asking again.
inline int pioran_grant_lds(std::initializer_list<LdsGrant> wanted)
{
    struct Grant {
        const void* kernel;
        size_t granted;   // the largest size the runtime has granted
        size_t refused;   // the smallest it has refused (SIZE_MAX: none)
    };
    static std::mutex mutex;                          // (an inline function's statics: one copy in the library)
    static std::vector<std::vector<Grant>> grants;    // [device ordinal]: the kernels asked for there, a few dozen at most
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) {
        (void)hipGetLastError();
        return PIORAN_ERR_HIP;
    }
    std::lock_guard<std::mutex> lock(mutex);
    if ((size_t)dev >= grants.size()) grants.resize((size_t)dev + 1);
    std::vector<Grant>& of_dev = grants[(size_t)dev];
    for (const LdsGrant& w : wanted) {
        if (!w.kernel) continue;
        Grant* g = nullptr;
        for (Grant& e : of_dev)
            if (e.kernel == w.kernel) { g = &e; break; }
        if (!g) {
            of_dev.push_back(Grant{w.kernel, 0, SIZE_MAX});
            g = &of_dev.back();
        }
        if (w.bytes <= g->granted) continue;
        if (w.bytes >= g->refused) return PIORAN_ERR_HIP;
        // (under the lock: a second thread with the same kernel waits for the answer instead of asking too)
        if (hipFuncSetAttribute(w.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)w.bytes) != hipSuccess) {
            (void)hipGetLastError();
            g->refused = w.bytes;
            return PIORAN_ERR_HIP;
        }
        g->granted = w.bytes;
    }
    return PIORAN_OK;
}
inline int pioran_grant_lds(const void* kernel, size_t bytes) { return pioran_grant_lds({LdsGrant{kernel, bytes}}); }
