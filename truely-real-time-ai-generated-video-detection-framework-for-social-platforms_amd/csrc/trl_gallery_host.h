// trl_gallery_host.h -- what the host entry points of trl_gallery.hip and trl_cluster.hip share.
#pragma once
#include "trl_common.h"

constexpr int CL_MAX_N = 65536;       // rows of a link bitmap: trl_cluster_links writes it, trl_cluster_labels reads it

// a caller's workspace is 8-byte aligned and held everything the entry carved from it (`carved`), else entry `who` refuses it and
// names need() bytes -- the entry's *_workspace function, run for the message only
template <typename Need>
bool trl_workspace_ok(const char* who, const void* d_ws, size_t ws_bytes, bool carved, Need&& need) {
    if (((uintptr_t)d_ws & 7) == 0 && carved) return true;
    trl_set_error("%s: workspace of %zu bytes (need %zu, 8-byte aligned)", who, ws_bytes, (size_t)need());
    return false;
}

// makes the device that holds `p` the current one
inline int trl_device_of(const void* p) {
    hipPointerAttribute_t attr;
    TRL_HIP(hipPointerGetAttributes(&attr, p));
    TRL_HIP(hipSetDevice(attr.device));
    return TRL_OK;
}
