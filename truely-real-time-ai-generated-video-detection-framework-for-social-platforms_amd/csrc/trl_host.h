// trl_host.h -- what the host entry points of the context-free files share (trl_gallery.hip, trl_cluster.hip, trl_tracks.hip,
// trl_pool.hip, trl_quality.hip, trl_shots.hip; trl_annotate.hip for the device lookup): how an entry refuses, which device it runs on, what it asks
// of a caller's workspace and of per-group state, and how a kernel with a large LDS frame is launched.
#pragma once
#include <string.h>

#include "trl_common.h"

// entry `who` refuses its arguments: "who: why"
inline int trl_refuse(const char* who, const char* why) {
    trl_set_error("%s: %s", who, why);
    return TRL_ERR_INVALID;
}

// makes the device that holds `p` the current one
inline int trl_device_of(const void* p) {
    hipPointerAttribute_t attr;
    TRL_HIP(hipPointerGetAttributes(&attr, p));
    TRL_HIP(hipSetDevice(attr.device));
    return TRL_OK;
}

// a caller's workspace is 8-byte aligned and held everything the entry carved from it (`carved`), else entry `who` refuses it and
// names need() bytes -- the entry's *_workspace function, run for the message only
template <typename Need>
bool trl_workspace_ok(const char* who, const void* d_ws, size_t ws_bytes, bool carved, Need&& need) {
    if (((uintptr_t)d_ws & 7) == 0 && carved) return true;
    trl_set_error("%s: workspace of %zu bytes (need %zu, 8-byte aligned)", who, ws_bytes, (size_t)need());
    return false;
}

// `p` is an 8-byte-aligned array of per-group state and there are 0 .. 2^31 - 1 groups, else entry `who` refuses.  `what` names the
// array in the messages, noun and verb: "state is", "keys are"
inline int trl_check_groups(const char* who, const char* what, const void* p, long long groups) {
    if (groups < 0 || groups > 0x7fffffffLL) return trl_refuse(who, "groups outside 0..2^31 - 1");
    if (!p) {
        trl_set_error("%s: null %.*s", who, (int)strcspn(what, " "), what);
        return TRL_ERR_INVALID;
    }
    if ((uintptr_t)p & 7) {
        trl_set_error("%s: the %s not 8-byte aligned", who, what);
        return TRL_ERR_INVALID;
    }
    return TRL_OK;
}

// a tile kernel's launch: 256 threads and `lds` bytes of dynamic LDS, which may lie above the default limit of 64 KB
template <typename... P, typename... A>
int trl_launch_lds(void (*kernel)(P...), long long wgs, size_t lds, hipStream_t s, A... args) {
    TRL_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kernel<<<(unsigned)wgs, 256, lds, s>>>(args...);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

// trl_pool.hip: d_key[0 .. groups) of trl_bestkey.h's keys -> the rows d_index and the scores d_score, for entry `who`, which calls
// the keys `what` (trl_check_groups); queued on `s`
int trl_best_key_read(const char* who, const char* what, const unsigned long long* d_key, long long groups, int32_t* d_index, float* d_score,
                      hipStream_t s);
