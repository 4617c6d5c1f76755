// conv3d_host.h -- host-side pieces shared by the conv translation units that launch persistent kernels
// (conv3d.hip, conv3d_up.hip, conv3d_wt.hip): the size of the persistent grid and the variant-name report.
#pragma once
#include "common.h"

namespace v2ce {
namespace {

// workgroups of a persistent launch: one per CU, a multiple of 8 so that a workgroup's tiles keep their XCD / L2
inline int persistent_cu_count() {
    static const int n_cu = [] {
        int dev = 0, n = 256;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            n = 256;
        return n < 8 ? 8 : (n / 8) * 8;
    }();
    return n_cu;
}

// (measured in the network, same box: 2200 vs 2143 frame-pairs/s against one tile per workgroup)
inline unsigned persistent_grid(long long blocks) {
    const int n_cu = persistent_cu_count();
    return (unsigned)(blocks > n_cu ? n_cu : blocks);
}

thread_local char *g_name_out = nullptr;   // non-null: a launcher reports its kernel's name instead of launching (the *_variant entries)
thread_local size_t g_name_cap = 0;

}  // namespace
}  // namespace v2ce
