// gact_walk_pos.hpp -- the running positions of the cooperative walk (coop_walk_batch, gact_coop.hpp), kept free of
// anything but integers so that a host compiler can build them too: tests/test_coop_walk_positions.py compiles this file
// and holds every function to the closed forms it replaces,
//     p = max(p0 + njs, 0), l = p / CW, c = p - l * CW;   position = pos0 + dir * n.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GACT_WALK_FN __host__ __device__ __forceinline__
#else
#define GACT_WALK_FN inline
#endif

namespace gact {

// The walk's column between two refills (a trip: at most eight moves, fewer than the CW > 8 columns of a lane) is kept
// relative to the lane the trip began in, l0: cr = c at the refill, one less for every move that consumed a query base,
// so cr < 0 says the walk is in lane l0 - 1, at column cr + CW.  cr_min = -CW * l0 is where p = l * CW + c is 0: the
// clamp of max(p0 + njs, 0), which only a trip that began in lane 0 can reach.
template <int CW>
GACT_WALK_FN void walk_trip_begin(int l, int c, int &cr, int &cr_min)
{
    cr = c;
#if defined(__HIP_DEVICE_COMPILE__)
    cr_min = __mul24(l, -CW);
#else
    cr_min = -CW * l;
#endif
}

// one move: dj = 1 if it consumed a query base (one column to the left), 0 changes nothing
GACT_WALK_FN void walk_col_left(int &cr, int cr_min, int dj)
{
    const int next = cr - dj;
    cr = next > cr_min ? next : cr_min;
}

// -1 in the lane before the trip's first, 0 in that lane: what the lane number and the stored step of the cell add
GACT_WALK_FN int walk_lane_before(int cr) { return cr >> 31; }

// (lane, column in lane) again, for the next refill
template <int CW>
GACT_WALK_FN void walk_trip_end(int l0, int cr, int &l, int &c)
{
    const int before = walk_lane_before(cr);
    l = l0 + before;
    c = cr + (before & CW);
}

// Twice the position in a staged slice after n steps (n <= 0) from pos0 in direction dir = +-1, as the bit offset of a
// 2-bit base: fix2 = 2 * pos0 (plus whatever base address the caller folds in), dir2 = 2 * dir.  One 24-bit
// multiply-add at full rate (|n| <= the tile size), where pos0 + dir * n in 32 bits is a 64-bit quarter-rate one.
GACT_WALK_FN int walk_pos2(int fix2, int dir2, int n)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(n, dir2) + fix2;
#else
    return n * dir2 + fix2;
#endif
}

}  // namespace gact
