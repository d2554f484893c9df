// Ticket order of the sweep launches: plain host arithmetic, no HIP and no grid object (GridT::xs_order and the
// device-free C entry ttcr_fsm_unit_order both call it; tests/test_unit_order.py checks what it promises).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

// Patches in anti-diagonal order, m = TJ + TK major (a topological order of the upwind dependencies inside a sweep):
// entries TJ | TK << 16.
inline std::vector<uint32_t> fsm_diag_order(int npj, int npk) {
    std::vector<uint32_t> order;
    order.reserve((size_t)npj * npk);
    for (int m = 0; m <= npj + npk - 2; ++m)
        for (int TK = std::max(0, m - npj + 1); TK <= std::min(m, npk - 1); ++TK)
            order.push_back((uint32_t)(m - TK) | ((uint32_t)TK << 16));
    return order;
}

// Ticket order of the whole-iteration launch: every unit (direction d, patch) once, entries TJ | TK << 14 | d << 28.
// A unit waits for its two upwind patches of the same sweep and for the patches of sweep d-1 that own a column
// within 2H of its own (fsm_sweep_persistent), so any order that puts those first is deadlock free whatever the
// number of resident workgroups.  by_time = false: sweep by sweep, anti-diagonals inside a sweep.  by_time = true:
// by the start time every unit would have on an unbounded machine (upwind patch + one hand-off; previous sweep's
// patches finished), in chunk times.  A sweep has more patches than the chip has workgroup slots; handed out sweep
// by sweep, the slots fill up with patches that sit out their turn on the ramp of the patch wavefront while the
// next sweep, whose first corner is long free, cannot enter.  In start-time order the resident units are the ones
// that can run next, of whichever sweep.
// NF, NJ, NK: nodes along the level axis and the two patch axes (2-D: NK = 1); PJ x PK: nodes of a patch; C: levels
// of a chunk; H: halo width of the stage (1: first order, 2: WENO); diag_order: fsm_diag_order of the patch grid.
inline std::vector<uint32_t> fsm_xs_order(int dim, int NF, int NJ, int NK, int PJ, int PK, int C, int H, bool by_time,
                                          const std::vector<uint32_t>& diag_order) {
    const int ndir = dim == 3 ? 8 : 4;
    const int npj = (NJ + PJ - 1) / PJ;
    const int n_patches = (int)diag_order.size();
    std::vector<uint32_t> out;
    out.reserve((size_t)n_patches * ndir);
    if (!by_time) {
        for (int d = 0; d < ndir; ++d)
            for (uint32_t e : diag_order) out.push_back((e & 0xffffu) | ((e >> 16) << 14) | ((uint32_t)d << 28));
        return out;
    }
    auto flags = [&](int d, int& rj, int& rk) {
        if (dim == 3) { rj = (d >> 1) & 1; rk = (d >> 2) & 1; } else { rj = (d == 1) | (d == 2); rk = 0; }
    };
    std::vector<double> ts((size_t)n_patches * ndir, 0.0), tf((size_t)n_patches * ndir, 0.0);
    const double hop_j = (PJ + C - 1.0) / C + 1.0, hop_k = (PK + C - 1.0) / C + 1.0;
    for (int d = 0; d < ndir; ++d) {
        int rj, rk, prj = 0, prk = 0;
        flags(d, rj, rk);
        if (d > 0) flags(d - 1, prj, prk);
        for (uint32_t e : diag_order) {
            const int TJ = e & 0xffffu, TK = e >> 16;
            const size_t me = (size_t)d * n_patches + (size_t)TK * npj + TJ;
            double t = 0.0;
            if (TJ > 0) t = std::max(t, ts[me - 1] + hop_j);
            if (TK > 0) t = std::max(t, ts[me - npj] + hop_k);
            const int j0 = TJ * PJ, k0 = TK * PK;
            const int jm = std::min(j0 + PJ, NJ) - 1, km = std::min(k0 + PK, NK) - 1;
            if (d > 0) {
                const int ja = std::max(j0 - 2 * H, 0), jb = std::min(jm + 2 * H, NJ - 1);
                const int ka = std::max(k0 - 2 * H, 0), kb = std::min(km + 2 * H, NK - 1);
                const int ja2 = rj != prj ? NJ - 1 - jb : ja, jb2 = rj != prj ? NJ - 1 - ja : jb;
                const int ka2 = rk != prk ? NK - 1 - kb : ka, kb2 = rk != prk ? NK - 1 - ka : kb;
                for (int tk = ka2 / PK; tk <= kb2 / PK; ++tk)
                    for (int tj = ja2 / PJ; tj <= jb2 / PJ; ++tj) t = std::max(t, tf[(size_t)(d - 1) * n_patches + (size_t)tk * npj + tj]);
            }
            ts[me] = t;
            tf[me] = t + ((jm - j0) + (km - k0) + NF + C - 1) / C + 1.0;
        }
    }
    std::vector<uint32_t> idx((size_t)n_patches * ndir);
    // stable sort by start time; ties keep (direction, anti-diagonal) order
    size_t q = 0;
    std::vector<uint32_t> ent((size_t)n_patches * ndir);
    std::vector<double> key((size_t)n_patches * ndir);
    for (int d = 0; d < ndir; ++d)
        for (uint32_t e : diag_order) {
            const int TJ = e & 0xffffu, TK = e >> 16;
            ent[q] = (uint32_t)TJ | ((uint32_t)TK << 14) | ((uint32_t)d << 28);
            key[q] = ts[(size_t)d * n_patches + (size_t)TK * npj + TJ];
            idx[q] = (uint32_t)q;
            ++q;
        }
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a2, uint32_t b2) { return key[a2] < key[b2]; });
    for (uint32_t i2 : idx) out.push_back(ent[i2]);
    return out;
}
