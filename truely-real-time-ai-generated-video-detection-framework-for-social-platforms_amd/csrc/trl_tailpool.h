// trl_tailpool.h -- geometry of the max pool that runs in a conv kernel's epilogue (R-Net conv2, O-Net conv2 / conv3).
// Integer arithmetic only: plain C++17, no HIP header, so a host compiler builds it for tests/tail_pool_sim.cpp.  The conv kernels
// (trl_layers.hip), the fix-up kernel and that program all call this one text.
//
// The conv's GEMM rows are the flattened (candidate, y, x) pixels of S x S maps, cut into tiles of BM rows that know nothing of
// maps or pooling windows.  A k x k / st window whose first element is row f covers rows f + ky S + kx: a span of (k-1) S + k rows,
// ascending in the pool's scan order (ky, then kx).  With span <= BM a window touches at most two consecutive tiles, the first
// holding a prefix of the scan and the second the rest.  Each tile reduces the part it holds ("part"): the tile with the window's
// first element writes its part to the pooled map, a second tile writes its part to a side buffer of the same shape, and the
// fix-up combines them as (B > A) ? B : A -- which equals the sequential scan, because the scan adopts a value only when it is
// strictly greater (the earliest of equal maxima wins, a NaN never does) and B is what the scan of the rest adopts from -inf.
//
// Cells are numbered g = (candidate P + py) P + px, as the pooled map stores them; first_row(g) ascends with g, so the cells a
// tile touches and the cells a tile boundary cuts are both contiguous ranges of g.
#pragma once

#if defined(__HIPCC__)
#define TRL_TP_FN __host__ __device__ __forceinline__ constexpr
#else
#define TRL_TP_FN inline constexpr
#endif

struct TailPool {
    int S, k, st, BM;       // conv output side, pool window and stride (no window is clipped: (S - k) % st == 0), rows per tile

    TRL_TP_FN int P() const { return (S - k) / st + 1; }          // pooled side
    TRL_TP_FN int per() const { return S * S; }                   // GEMM rows per candidate
    TRL_TP_FN int cells() const { return P() * P(); }             // pooled cells per candidate
    TRL_TP_FN int span() const { return (k - 1) * S + k; }        // rows from a window's first element to its last, inclusive
    // the fused form applies: whole windows only, and no window longer than a tile
    TRL_TP_FN bool ok() const { return S >= k && k >= 1 && st >= 1 && (S - k) % st == 0 && span() <= BM; }
    // no window can meet a tile boundary: tiles are whole candidates
    TRL_TP_FN bool can_straddle() const { return BM % per() != 0; }

    // row of the first element of cell g's window
    TRL_TP_FN int first_row(int g) const {
        const int cand = g / cells(), c = g - cand * cells();
        const int py = c / P(), px = c - py * P();
        return cand * per() + py * st * S + px * st;
    }
    // the smallest g whose window starts at row r or later (r < 0 counts as 0)
    TRL_TP_FN int cell_from(int r) const {
        if (r <= 0) return 0;
        const int cand = r / per(), rem = r - cand * per();
        const int y = rem / S, x = rem - y * S;
        int py = (y + st - 1) / st, px = 0;
        if (py * st == y) {                                        // windows start in this map row: the first at column >= x
            px = (x + st - 1) / st;
            if (px >= P()) { px = 0; py++; }
        }
        if (py >= P()) return (cand + 1) * cells();                // none left in this map
        return cand * cells() + py * P() + px;
    }
    // tile t (rows t BM .. t BM + BM - 1) holds an element of cells tile_cell0(t) .. tile_cell1(t) - 1, and of no other
    TRL_TP_FN int tile_cell0(int t) const { return cell_from(t * BM - span() + 1); }
    TRL_TP_FN int tile_cell1(int t) const { return cell_from(t * BM + BM); }
    // its part of cell g is the window's SECOND part (side buffer) when the first element lies in the tile before
    TRL_TP_FN bool second_part(int g, int t) const { return first_row(g) < t * BM; }
    // cell g has two parts
    TRL_TP_FN bool straddles(int g) const { return first_row(g) / BM != (first_row(g) + span() - 1) / BM; }
    // the cells cut by the boundary in front of tile b (b >= 1): cut_cell0(b) .. cut_cell1(b) - 1; over all b, every straddling cell once
    TRL_TP_FN int cut_cell0(int b) const { return cell_from(b * BM - span() + 1); }
    TRL_TP_FN int cut_cell1(int b) const { return cell_from(b * BM); }
};
