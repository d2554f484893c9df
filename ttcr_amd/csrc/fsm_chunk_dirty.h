// Chunk-shaped dirty bits of the first-order 3-D kernels with exact skipping (fsm_sweep_unit, "CD"): which chunks of the NEXT sweep read
// a node that changed in this one.  Plain arithmetic shared by the kernel and the device-free C entry ttcr_fsm_chunk_dirty_marks
// (tests/test_chunk_dirty_marks.py checks what it promises; DESIGN.md section 4a has the argument).
//
// A sweep in direction dn (bits: F, J, K reversed) walks oriented indices (i', j', k'); unit (TJ, TK) owns the PJ x PK patch of (j', k')
// columns of dn's own partition and evaluates its nodes by level l = i' + j' + k' in chunks of C levels, the first of which starts at
//     lcf = Ls - ((Ls - (TJ + TK)) mod C),   Ls = TJ PJ + TK PK
// (chunk starts are congruent to TJ + TK modulo C).  A node is read by its six axis neighbours only: they sit at levels l - 1 and l + 1, in
// the node's own column (F neighbours) or in a column one step away along J or K -- the node's own patch, or, for a column within H of
// a patch edge, the patch beyond that edge (never a diagonal one).
//
// Two steps, because the kernel takes them at different times: the units a COLUMN marks, with what is needed to turn an F index into a
// chunk of theirs (once per work unit and thread, kept in LDS), and the chunks of one of those units for a run of nodes of the column
// (once per chunk in which the thread changed a node).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FSM_CD_HD __host__ __device__ __forceinline__
#else
#define FSM_CD_HD inline
#endif

// first chunk start of unit (TJ, TK)
FSM_CD_HD int fsm_chunk_first(int TJ, int TK, int PJ, int PK, int C) {
    const int Ls = TJ * PJ + TK * PK;
    return Ls - (((Ls - (TJ + TK)) % C + C) % C);
}

// The units of the sweep in direction dn that read a node of the NATURAL column (jn, kn): emit(TJ, TK, rel, nch) once per unit -- the
// column's own unit first, then the units beyond a patch edge the column lies within H of (edge_rule = false leaves those out: the
// negative control of the tests).  rel = lcf - (j' + k') of the column in dn's orientation: the node with oriented F index i' sits in
// chunk (i' - rel) / C of that unit's chunk grid; nch: chunks of the unit (levels lcf .. Le).
template <class Emit>
FSM_CD_HD void fsm_chunk_mark_units(int NF, int NJ, int NK, int PJ, int PK, int C, int H, int dn, int jn, int kn, bool edge_rule, Emit&& emit) {
    const int rj = (dn >> 1) & 1, rk = (dn >> 2) & 1;
    const int j2 = rj ? NJ - 1 - jn : jn, k2 = rk ? NK - 1 - kn : kn;
    const int TJ = j2 / PJ, TK = k2 / PK;
    auto one = [&](int tj, int tk) {
        const int j0 = tj * PJ, k0 = tk * PK;
        const int jm = (j0 + PJ < NJ ? j0 + PJ : NJ) - 1, km = (k0 + PK < NK ? k0 + PK : NK) - 1;
        const int lcf = fsm_chunk_first(tj, tk, PJ, PK, C);
        emit(tj, tk, lcf - (j2 + k2), (jm + km + NF - 1 - lcf) / C + 1);
    };
    one(TJ, TK);
    if (edge_rule) {
        if (TJ > 0 && j2 - H < TJ * PJ) one(TJ - 1, TK);
        if ((TJ + 1) * PJ < NJ && j2 + H >= (TJ + 1) * PJ) one(TJ + 1, TK);
        if (TK > 0 && k2 - H < TK * PK) one(TJ, TK - 1);
        if ((TK + 1) * PK < NK && k2 + H >= (TK + 1) * PK) one(TJ, TK + 1);
    }
}

// Chunks *c0 .. *c1 of a unit (rel, nch from fsm_chunk_mark_units) that hold the levels l - 1 .. l + 1 of the nodes with NATURAL F indices
// fa .. fb of the column, clipped to the unit's chunks; false: none.  A superset of the readers' chunks, never less.
FSM_CD_HD bool fsm_chunk_mark_range(int NF, int C, int dn, int rel, int nch, int fa, int fb, int* c0, int* c1) {
    const int rf = dn & 1;
    const int ia = (rf ? NF - 1 - fb : fa) - 1 - rel, ib = (rf ? NF - 1 - fa : fb) + 1 - rel;
    const int a = ia < 0 ? 0 : ia / C, b = ib < 0 ? -1 : (ib / C < nch - 1 ? ib / C : nch - 1);
    *c0 = a;
    *c1 = b;
    return a <= b;
}

// Both steps for one run of nodes: emit(TJ, TK, c0, c1) per unit that reads one of them.
template <class Emit>
FSM_CD_HD void fsm_chunk_marks(int NF, int NJ, int NK, int PJ, int PK, int C, int H, int dn, int jn, int kn, int fa, int fb,
                               bool edge_rule, Emit&& emit) {
    fsm_chunk_mark_units(NF, NJ, NK, PJ, PK, C, H, dn, jn, kn, edge_rule, [&](int tj, int tk, int rel, int nch) {
        int c0, c1;
        if (fsm_chunk_mark_range(NF, C, dn, rel, nch, fa, fb, &c0, &c1)) emit(tj, tk, c0, c1);
    });
}
