// trl_redzone.hip -- red zones behind every block of a context's two workspaces (trl_debug_redzone, include/truely_hip.h): the sweep
// kernel, its bookkeeping and the three hooks.  Off unless a test turns it on; the product path reaches it through trl_rz_end and
// trl_ensure (trl_ctx.h) only while it is on.
#include <string.h>
#include <algorithm>

#include "trl_ctx.h"

// One workgroup column per gap: res[3 g] += bytes of gap g that differ from `byte`, res[3 g + 1] / [3 g + 2] = min / max of their
// offsets within the gap.  gaps[2 g] / [2 g + 1] = the gap's offset in the workspace and its length.  Reads only, all inside the gap.
__global__ void k_rz_scan(const unsigned char* __restrict__ base, const unsigned long long* __restrict__ gaps, unsigned long long* __restrict__ res,
                          int g0, unsigned byte) {
    const int g = g0 + blockIdx.y;
    const unsigned long long len = gaps[2 * g + 1];
    const unsigned char* p = base + gaps[2 * g];
    unsigned long long head = (16 - ((uintptr_t)p & 15)) & 15;            // bytes in front of the first aligned 16
    if (head > len) head = len;
    const unsigned long long nw = (len - head) / 16, tail0 = head + nw * 16;
    const unsigned long long w = 0x0101010101010101ull * (byte & 0xFF);
    const unsigned long long tid = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x, nt = (unsigned long long)gridDim.x * blockDim.x;
    unsigned long long cnt = 0, first = ~0ull, last = 0;
    auto look = [&](unsigned long long i) {
        if (p[i] == (unsigned char)byte) return;
        cnt++;
        if (i < first) first = i;
        if (i > last) last = i;
    };
    if (tid == 0) {
        for (unsigned long long i = 0; i < head; i++) look(i);
        for (unsigned long long i = tail0; i < len; i++) look(i);
    }
    const ulonglong2* q = reinterpret_cast<const ulonglong2*>(p + head);
    for (unsigned long long k = tid; k < nw; k += nt) {
        const ulonglong2 v = q[k];
        if (v.x == w && v.y == w) continue;
        for (int b = 0; b < 16; b++) look(head + k * 16 + b);
    }
    if (cnt) {
        atomicAdd(&res[3 * g], cnt);
        atomicMin(&res[3 * g + 1], first);
        atomicMax(&res[3 * g + 2], last);
    }
}

namespace {
struct RzGap { size_t off, len; int block; size_t block_bytes; };
// every stretch of `a` that belongs to no block: behind each live block up to the next one (the last: up to a.off), then the tail
void rz_gaps(const Arena& a, std::vector<RzGap>& out) {
    const size_t nb = a.blocks.size();
    for (size_t i = 0; i < nb; i++) {
        const size_t end = a.blocks[i].off + a.blocks[i].bytes, next = i + 1 < nb ? a.blocks[i + 1].off : a.off;
        if (next > end) out.push_back({end, next - end, (int)i, a.blocks[i].bytes});
    }
    if (a.cap > a.off) out.push_back({a.off, a.cap - a.off, (int)nb, 0});
}
// The sweep of one workspace.  refill_from >= 0 (a rewind to that offset): everything from there to the capacity is refilled
int rz_sweep(trl_ctx* c, Arena& a, const char* site, long long refill_from) {
    Hooks::RedZone& z = c->hook.rz;
    TRL_HIP(hipDeviceSynchronize());             // the call's stream, and every other one
    if (!a.base) return TRL_OK;
    std::vector<RzGap> gaps;
    rz_gaps(a, gaps);
    const size_t ng = gaps.size();
    if (ng) {
        if (z.dev_gaps < ng) {
            if (z.dev) TRL_HIP(hipFree(z.dev));
            z.dev = nullptr; z.dev_gaps = 0;
            TRL_HIP(hipMalloc((void**)&z.dev, (ng + 256) * 5 * 8));
            z.dev_gaps = ng + 256;
        }
        std::vector<unsigned long long> tab(5 * ng, 0);
        for (size_t g = 0; g < ng; g++) { tab[2 * g] = gaps[g].off; tab[2 * g + 1] = gaps[g].len; tab[2 * ng + 3 * g + 1] = ~0ull; }
        TRL_HIP(hipMemcpy(z.dev, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
        // the gaps behind blocks are a guard long: a few workgroups each, 32 K gaps per launch; the tail (last) is the long one
        const bool has_tail = gaps.back().block == (int)a.blocks.size();
        const size_t nshort = has_tail ? ng - 1 : ng;
        for (size_t g0 = 0; g0 < nshort; g0 += 32768) {
            const unsigned ny = (unsigned)std::min<size_t>(32768, nshort - g0);
            k_rz_scan<<<dim3(4, ny), 256>>>((const unsigned char*)a.base, z.dev, z.dev + 2 * ng, (int)g0, (unsigned)z.byte);
            TRL_LAUNCH_CHECK();
        }
        if (has_tail) {
            k_rz_scan<<<dim3(4096, 1), 256>>>((const unsigned char*)a.base, z.dev, z.dev + 2 * ng, (int)(ng - 1), (unsigned)z.byte);
            TRL_LAUNCH_CHECK();
        }
        TRL_HIP(hipMemcpy(tab.data() + 2 * ng, z.dev + 2 * ng, 3 * ng * 8, hipMemcpyDeviceToHost));
        for (size_t g = 0; g < ng; g++) {
            z.bytes += (long long)gaps[g].len;
            const unsigned long long* r = &tab[2 * ng + 3 * g];
            if (!r[0]) continue;
            z.nhits++;
            if (z.hits.size() < TRL_RZ_MAX_HITS) {
                trl_rz_hit h;
                memset(&h, 0, sizeof h);
                h.arena = &a == &c->arena ? 0 : 1; h.block = gaps[g].block;
                strncpy(h.site, site, sizeof(h.site) - 1);
                h.block_bytes = (long long)gaps[g].block_bytes; h.gap_off = (long long)gaps[g].off; h.gap_bytes = (long long)gaps[g].len;
                h.first = (long long)r[1]; h.last = (long long)r[2]; h.count = (long long)r[0];
                z.hits.push_back(h);
            }
            TRL_HIP(hipMemset(a.base + gaps[g].off, z.byte, gaps[g].len));   // repaired: reported once
        }
    }
    z.sweeps++;
    if (refill_from >= 0 && (size_t)refill_from < a.cap) TRL_HIP(hipMemset(a.base + refill_from, z.byte, a.cap - (size_t)refill_from));
    TRL_HIP(hipDeviceSynchronize());
    return TRL_OK;
}
// Arena::on_rewind of the two workspaces while the guard is on (a failing HIP call here fails the next one of the entry point too)
void rz_on_rewind(Arena& a, size_t mark, const char* site, void* owner) { (void)rz_sweep((trl_ctx*)owner, a, site, (long long)mark); }
}  // namespace

int trl_rz_sweep(trl_ctx* c, const char* site, Arena* one) {
    if (one) return rz_sweep(c, *one, site, -1);
    TRL_CHECK(rz_sweep(c, c->arena, site, -1));
    return rz_sweep(c, c->scratch, site, -1);
}

extern "C" {

int trl_debug_redzone(trl_ctx* c, long long guard, int byte) {
    TRL_CHECK(trl_hook_device(c));
    if (guard < 0 || guard > TRL_RZ_MAX_GUARD || (guard & 255) || byte < 0 || byte > 255) {
        trl_set_error("bad red zone: guard %lld (0, or a multiple of 256 up to %d), fill byte %d", guard, (int)TRL_RZ_MAX_GUARD, byte);
        return TRL_ERR_INVALID;
    }
    Hooks::RedZone& z = c->hook.rz;
    if (!guard && !z.guard) return TRL_OK;
    TRL_HIP(hipDeviceSynchronize());
    if (!z.guard) z.saved_poison = c->hook.dbg_poison;
    // both workspaces start over, so that every byte of them is filled by trl_ensure and every block is known
    for (Arena* a : {&c->arena, &c->scratch}) {
        if (a->base) TRL_HIP(hipFree(a->base));
        a->base = nullptr; a->cap = a->off = a->high = 0;
        a->blocks.clear();
        a->guard = (size_t)guard; a->on_rewind = guard ? rz_on_rewind : nullptr; a->owner = c;
    }
    c->cb = CascadeBufs();
    c->arena_need = 0;
    c->fn_need_key[0] = 0;                       // the embedder's count depends on the guard
    z.guard = (size_t)guard; z.byte = byte;
    z.sweeps = z.bytes = z.nhits = 0;
    z.hits.clear();
    c->hook.dbg_poison = guard ? byte : z.saved_poison;
    return TRL_OK;
}

int trl_debug_redzone_report(trl_ctx* c, int flags, long long* h_out4, trl_rz_hit* h_hits, int max_hits) {
    TRL_CHECK(trl_hook_device(c));
    if (!h_out4 || (max_hits > 0 && !h_hits)) { trl_set_error("null argument"); return TRL_ERR_INVALID; }
    Hooks::RedZone& z = c->hook.rz;
    if ((flags & TRL_RZ_SWEEP) && z.guard) TRL_CHECK(trl_rz_sweep(c, "report"));
    int m = 0;
    for (; m < (int)z.hits.size() && m < max_hits; m++) h_hits[m] = z.hits[m];
    h_out4[0] = z.sweeps; h_out4[1] = z.bytes; h_out4[2] = z.nhits; h_out4[3] = m;
    if (flags & TRL_RZ_CLEAR) { z.sweeps = z.bytes = z.nhits = 0; z.hits.clear(); }
    return TRL_OK;
}

int trl_debug_redzone_poke(trl_ctx* c, int arena, int block, long long offset, int value) {
    TRL_CHECK(trl_hook_device(c));
    Hooks::RedZone& z = c->hook.rz;
    if (!z.guard) { trl_set_error("red zones are off"); return TRL_ERR_STATE; }
    if ((arena != 0 && arena != 1) || value < 0 || value > 255 || value == z.byte) { trl_set_error("bad argument"); return TRL_ERR_INVALID; }
    Arena& a = arena ? c->scratch : c->arena;
    if (!a.base) { trl_set_error("the workspace has not been allocated"); return TRL_ERR_STATE; }
    std::vector<RzGap> gaps;
    rz_gaps(a, gaps);
    if (block < 0) block = (int)a.blocks.size();                            // the tail
    for (const RzGap& g : gaps) {
        if (g.block != block) continue;
        if (offset < 0 || (size_t)offset >= g.len) break;
        TRL_HIP(hipDeviceSynchronize());
        TRL_HIP(hipMemset(a.base + g.off + (size_t)offset, value, 1));    // inside [0, cap): a gap of this workspace
        TRL_HIP(hipDeviceSynchronize());
        return TRL_OK;
    }
    trl_set_error("no byte %lld in the gap behind block %d (%zu live blocks)", offset, block, a.blocks.size());
    return TRL_ERR_INVALID;
}

}  // extern "C"
