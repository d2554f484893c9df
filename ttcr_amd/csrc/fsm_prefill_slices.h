// Slices of the spare traveltime fields that the units of a sweep launch fill with max() (PersistArgs::fill_dst, fsm_sweep_unit;
// host side: GridT::solve_batch): plain arithmetic shared by the kernel, the host and the device-free C entry
// ttcr_fsm_prefill_slice (tests/test_prefill_slices.py checks what it promises).
#pragma once
#include <cstddef>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FSM_SLICE_HD __host__ __device__
#else
#define FSM_SLICE_HD
#endif

// Elements of one ticket's slice: n_el elements spread over n_tickets tickets, rounded up to whole 16-byte vectors (vec elements:
// 4 fp32, 2 fp64), so that every slice starts on a vector boundary of an aligned buffer.  Never 0 (0 means "no fill" to the kernel).
FSM_SLICE_HD inline size_t fsm_fill_slice_len(size_t n_el, size_t n_tickets, size_t vec) {
    if (n_tickets == 0) n_tickets = 1;
    const size_t per = (n_el + n_tickets - 1) / n_tickets;
    const size_t len = (per + vec - 1) / vec * vec;
    return len ? len : vec;
}

// Slice of `ticket`: elements [*b, *e) of [0, n_el).  Every ticket of a launch is drawn exactly once, so tickets 0 .. n_tickets-1
// cover the range exactly: consecutive, no gap, no overlap; the last non-empty slice ends at n_el whether or not that is a multiple
// of the vector (the tail).  A ticket whose slice would start at or beyond n_el -- the tickets past the unit count among them, since
// n_tickets * slice >= n_el -- covers nothing (*b == *e).
FSM_SLICE_HD inline void fsm_fill_slice_range(size_t n_el, size_t slice, size_t ticket, size_t* b, size_t* e) {
    // (a product that does not fit lies beyond n_el)
    size_t lo;
    if (__builtin_mul_overflow(ticket, slice, &lo)) lo = n_el;
    const size_t b_ = lo < n_el ? lo : n_el;
    const size_t e_ = n_el - b_ < slice ? n_el : b_ + slice;
    *b = b_;
    *e = e_;
}
