// gact_lin.hpp -- the packed-int16 chain pass for LINEAR gap scoring: gap_open == gap_extend == mismatch =: g
// (the reference's own params.cfg: +1 / -1 / -1 / -1), 2-bit read sets.  Same cells, same results as
// dp_pass_p16s / dp_pass_p16 -- fewer instructions per cell: 6 instead of 11 per cell pair for the scores,
// 10 instead of 22 where pointers are made, and pointers of 2 bits per cell instead of 4.
//
// 1. H alone.  The reference keeps M, I, D (align.cpp:134-160): I[i][j] = max(M, I)[i-1][j] + g.  That differs from
//    H[i-1][j] + g only where D is the strict maximum at (i-1, j), and then
//      H[i-1][j] + g = D[i-1][j] + g <= H[i-1][j-1] + 2g <= H[i-1][j-1] + mismatch <= M[i][j]:
//    the difference never reaches H[i][j], nor the choice between M, I and D there (M wins a tie, align.cpp:162-164).
//    The same for D.  So one value per cell is carried,
//      H[i][j] = max(M, 0, H[i-1][j] + g, H[i][j-1] + g),        M = H[i-1][j-1] + sub,
//    and every H, every op and every arg-max is the reference's.
// 2. Drifted frames.  A value is kept as X + (a frame that grows by |g| per row), so that H[i-1][j] + g is the upper
//    neighbour as it stands.  The frame is tied to the step, not to the tile's row number (rows in front of row 1 are
//    virtual and behave like row 0, gact_device.hpp), so two tiles with different start delays share it.
//    a. Row drift (the uniform pass, dp_pass_lin: seed and wide launches).  Every value of DP row i is X + beta_i with
//       beta_i = -i * g: the zero level is Z = beta_i, one register per lane moved by one v_add per step, and
//       M' = H'_diag + (sub - g) where sub - g is 0 for a mismatch (mismatch == g) and match - g otherwise: the
//       non-negative byte the look-up word of dp_pass_p16 already holds.  H_left + g costs a subtraction per column slot
//       on the serial chain.  Per cell pair: perm, add | max3 (Z, H'_up) | sub, max = 5 instructions (5. below).
//    b. Column drift (the split pass, dp_pass_lin_split_col, round 9; dp_pass_lin_split keeps the row drift for the
//       scorings of 12. below).  The cell a lane computes at step t in column slot c
//       is kept as X + Zw(t + c), Zw(k) = lin_base + k |g|: the frame grows along the columns of a lane too, so
//       H_left + g is the left neighbour of the same lane AS IT STANDS -- the subtraction is gone, the serial chain of
//       an untagged slot is one v_pk_max_i16 -- and the diagonal, two gaps below, gets its 2|g| from the look-up word
//       (lin_lut_fill_col, gact_p16.hpp: |g| for a mismatch, match + 2|g| for a match).  The frame depends on the step
//       and the slot only, not on the lane, the tile or the row: the zero level of (t, c) is ONE number for the wave.
//       A window of them, W[k] = Zw(t - 1 + k) for k = 0 .. C2 + 1, serves region 1 (slot c: W[c + 1]), region 2 (the
//       same) and the j = 0 border (W[0]: one gap below slot 0's level); the pointer phase keeps T[c] = 4 Zw(t + c) + 3
//       for region 2.  They live in SGPRs, move by one s_add_u32 each per step (both half-words at once: every value is
//       positive and far from a carry; inside whole blocks of steps they do not move at all, 13. below) and enter the cell as the scalar operand of the v_pk_maximum3_f16 that is there
//       anyway.  A value that crosses a lane changes frames by a constant, folded into the DPP hand-over (11. below):
//       (C1 - 1)|g| between lanes of region 1 and from lane 15's region 1 into lane 0's region 2 (scaled by four with
//       the tag in the addend of the v_pk_mad_u16 of the pointer phase), (C2 - 1)|g| between lanes of region 2.  Slot
//       0's diagonal is last step's hand-over value as before.  A pad row's words and a pad column's constant stay 0:
//       both only ever lower a value that the zero level clamps.  Per cell pair: perm, add | max3 | max = 4
//       instructions, 8 where pointers are made (the subtraction there is also the re-tag 2 -> 1 and became - 1).
//       tests/test_lin_col_drift_model.py runs this at lane level against the plain recurrence and holds the value range
//       and the byte rule (12.) over every scoring p16_lin_ok admits at every tile the layout runs.
// 3. Op-only pointers.  Inside the traceback window the scores are times four and the two low bits say where a value
//    came from -- M 3, H_up 2, H_left 1: the numbering of align.h:23, and the tie order of align.cpp:162-164 is the
//    order of the tags:
//      H'' = max(M'' | 3, Z'', H''_up - 1, H''_left - (4|g| + 2)),     op = H'' & 3,     stored: G = H'' | 3
//    (as of round 3 the stored form is G = (H'' & ~3) | 2 -- it is H''_up - 1 as it stands -- with the diagonal's tag
//    coming from a +1 in the look-up word and the left neighbour's from 4|g| + 1: see dp_pass_lin_split)
//    -- 10 instructions per pair with the two that shift the op into its column's half-word.  No open / extend flags
//    are made: the walker does not need them (walk_chain_lin, gact_chain.hpp: with these scorings the next state of
//    the traceback is the op of the cell it enters).  H == 0 shows as op 3 like MATCH (M'' is clamped to the zero
//    level tagged 3): ZERO is left to the walker too, which carries the score of the cell it stands on.  It needs H
//    of the start cell (R, Q): every tile of a wave is delayed so that its last row falls on the wave's last step,
//    and the value is simply what the lane of column Q holds when the loop ends.
// 4. Instruction classes.  tools/issue_probe.hip (profiles/r02/issue_rate_probe.json): with three waves on a SIMD
//    v_add_u32 / v_sub_u32 / v_and_b32 / v_or_b32 on VGPR operands issue every 1.9 cycles, v_pk_*, v_max_*,
//    v_perm_b32, v_mad_*, DPP moves and anything with an SGPR operand every 3.2-3.4.  So the frame is shifted up
//    (lin_base) until every value is a positive int16: the packed additions then cannot carry or borrow across the
//    half-words and run as plain 32-bit v_add_u32 / v_sub_u32, the re-taggings are a subtraction each, and the
//    constants of fast-class instructions sit in VGPRs (vconst).  An instruction that is in the slow class anyway takes
//    a wave-uniform operand out of an SGPR for nothing: the zero levels of the column-drifted split pass (2b.) are operands of its
//    v_pk_maximum3_f16 and are kept and moved by the scalar unit, off the VALU and out of the VGPR file.
#pragma once

#include <type_traits>

#include "gact_p16s.hpp"

namespace gact {

// 5. One instruction for two of the three maxima.  Every value of the pass is a positive int16 below 0x7C00, and positive
//    IEEE half-precision numbers order exactly like their bit patterns: max(M', Z, H'_up) -- off the serial column chain --
//    is ONE v_pk_maximum3_f16 (gfx950) where the integer instruction set needs two v_pk_max_i16.  The maximum returns one
//    of its operands bit for bit (no NaN below 0x7C00; lin_base keeps every value at or above 0x0400, a normal number,
//    whatever the denormal mode).  5 instructions per cell pair for the scores, 9 where pointers are made; the slow
//    instruction class (3.2 cycles at three waves) goes from 4 to 3 / from 5 to 4 of them.
#ifndef GACT_LIN_MAX3
#define GACT_LIN_MAX3 1
#endif
constexpr int kLinFloor = GACT_LIN_MAX3 ? 1024 : 0;
// zero level of lane 0 before step 1: above 31 lanes' worth of drift plus one gap, so nothing ever goes below |g|
// (below kLinFloor + |g|)
__host__ __device__ constexpr int lin_base(int g) { return kLinFloor + 40 * (-g) + 8; }
// a wave-uniform constant the compiler must keep in a VGPR (an SGPR operand would put the instruction in the slow class)
__device__ __forceinline__ uint32_t vconst(uint32_t s)
{
    uint32_t r;
    asm volatile("s_nop 1\n\tv_mov_b32 %0, %1" : "=v"(r) : "s"(s));     // (wait states: s may come out of a spill lane)
    return r;
}

// every score, times four, plus the drift of up to kMaxSteps + lanes + lag rows must fit int16
__host__ inline bool p16_lin_ok(int tile, int match, int mismatch, int open, int ext)
{
    const long long steps = (long long)tile + 4 * kGroup + 64 + 48;        // drift of the longest pass + lin_base
    return open == ext && mismatch == ext && ext <= 0 && match >= 0 &&
           p16_tagged_ok(tile, match, mismatch, open, ext) &&
           4 * ((long long)match * (tile + 2) + (long long)(-ext) * steps + kLinFloor) + 3 <= 30000 && match - ext <= 63;
}

// 10. Builtins in place of inline assembly (round 7): a switch, off.  Between an inline-asm VALU instruction and a VALU
//     instruction that reads its result the hazard recogniser puts an s_nop 0: it cannot see that the instruction has no
//     dst-forwarding hazard.  With GACT_LIN_BUILTINS=1 the helpers of the linear-gap passes that still come out as the ONE
//     instruction meant are builtins or vector expressions (v_pk_max_i16, v_bitop3_b32, v_pk_sub_i16, v_pk_ashrrev_i16;
//     stages and scheduling barriers as they were): VALU counts are the same and the s_nop per step fall to a third.  Not
//     v_pk_mad_u16 a, 4, c (a shift and an addition as a vector expression) and not v_pk_maximum3_f16 (three more VALU
//     instructions per remainder step, one per seed step).  Off because the split kernel then spills two SGPRs more than
//     with the inline-asm forms, whichever of the helpers is switched; what it does to the time: DESIGN 5, round 7.
#ifndef GACT_LIN_BUILTINS
#define GACT_LIN_BUILTINS 0
#endif
// 12. Which split pass runs.  The column-drifted pass's look-up byte of the pointer phase is 4 (match + 2|g|) + 1 and must
//     fit 255: match + 2|g| <= 63, where p16_lin_ok admits match + |g| <= 63.  At tile 320 every admitted scoring fits;
//     SplitLayoutLin<7, 13> also runs smaller tiles, and at tile 64 (62, -1, -1, -1) is admitted and does not.  The guard is
//     not narrowed and the plan does not change: the launch takes the same kernel on the row-drifted pass
//     (SplitLayoutLinRow, dp_pass_lin_split) for a scoring that fails lin_col_drift_ok, the column-drifted one otherwise.
//     The value range needs no rule of its own: the frame adds at most (C2 - 1)|g| to the row drift and lin_base, inside
//     what p16_lin_ok allows at every tile (tests/test_lin_col_drift_model.py).
//     Two things in how the column-drifted pass is written came from measuring it.  It takes the builtin
//     forms of v_pk_max_i16 and v_bitop3_b32 (kLinSplitBuiltins): with the subtraction gone an untagged slot's chain is
//     maximum after maximum, and after an inline-asm one the hazard recogniser puts an s_nop 0 in front of each; the other
//     passes keep 10.'s switch, so the seed and wide kernels are as they were.  And in the pointer phase its zero levels move
//     by an s_add_u32 the compiler cannot see through: written in C++ the compiler keeps every level as a loop-invariant base
//     plus a running offset, twice the scalar registers, with lane-spill reads inside the pointer phase's block loops.  On
//     plain scores the C++ form is the better one (opaque, the single step behind the two-step loop becomes a loop of its own).
__host__ inline bool lin_col_drift_ok(int match, int ext) { return match - 2 * ext <= 63; }
constexpr bool kLinSplitBuiltins = true;
typedef short LinS2 __attribute__((ext_vector_type(2)));
template <bool BUILTIN = GACT_LIN_BUILTINS>
__device__ __forceinline__ uint32_t lin_max(uint32_t a, uint32_t b)        // pk_max (v_pk_max_i16)
{
    if constexpr (BUILTIN)
        return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(LinS2, a), __builtin_bit_cast(LinS2, b)));
    else
        return pk_max(a, b);
}
__device__ __forceinline__ uint32_t lin_sub(uint32_t a, uint32_t b)        // pk_sub (v_pk_sub_i16)
{
#if GACT_LIN_BUILTINS
    return __builtin_bit_cast(uint32_t, (LinS2)(__builtin_bit_cast(LinS2, a) - __builtin_bit_cast(LinS2, b)));
#else
    return pk_sub(a, b);
#endif
}
__device__ __forceinline__ uint32_t pk_mad4v(uint32_t a, uint32_t v_c)     // a * 4 + c (wrapping halves), c in a VGPR
{
    uint32_t r;
    asm("v_pk_mad_u16 %0, %1, 4, %2 op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "v"(v_c));
    return r;
}
// max of three positive int16 pairs as half-precision numbers (see 5. above)
__device__ __forceinline__ uint32_t pk_max3f(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t r;
    asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// the same with the middle operand out of an SGPR (the instruction is in the slow class as it is: the scalar operand is free)
__device__ __forceinline__ uint32_t pk_max3f_s(uint32_t a, uint32_t s_b, uint32_t c)
{
    uint32_t r;
    asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(s_b), "v"(c));
    return r;
}
__device__ __forceinline__ uint32_t pk_max_sgpr(uint32_t a, uint32_t s_b)
{
    uint32_t r;
    asm("v_pk_max_i16 %0, %1, %2" : "=v"(r) : "v"(a), "s"(s_b));
    return r;
}
// 11. Hand-overs of the column-drifted split pass (2b. above): a lane takes its left neighbour's last slot less a constant
//     of the frame, the subtraction riding on the DPP move (v_sub_u32_dpp: a lane without a source keeps what the register
//     held).  A DPP operand written by the VALU needs two wait states, and the compiler does not look into an asm
//     statement: every statement keeps them itself, with the instructions that do not read across lanes where it can.
#define GACT_DPP_SHR1 " row_shr:1 row_mask:0xf bank_mask:0xf"
#define GACT_DPP_ROR1 " row_ror:1 row_mask:0xf bank_mask:0xf"
// lane n: h[n - 1] - k, lane 0 of a row: s_old
__device__ __forceinline__ uint32_t lin_hand_shr1(uint32_t h, uint32_t v_k, uint32_t s_old)
{
    uint32_t r;
    asm("v_mov_b32 %0, %3\n\ts_nop 0\n\tv_sub_u32_dpp %0, %1, %2" GACT_DPP_SHR1 : "=&v"(r) : "v"(h), "v"(v_k), "s"(s_old));
    return r;
}
// lane n: h2[n - 1] - k2, lane 0 of a row: h1[15] - k1
__device__ __forceinline__ uint32_t lin_hand_ror1_shr1(uint32_t h1, uint32_t v_k1, uint32_t h2, uint32_t v_k2)
{
    uint32_t r;
    asm("s_nop 1\n\tv_sub_u32_dpp %0, %1, %2" GACT_DPP_ROR1 "\n\tv_sub_u32_dpp %0, %3, %4" GACT_DPP_SHR1
        : "=&v"(r) : "v"(h1), "v"(v_k1), "v"(h2), "v"(v_k2));
    return r;
}
// what lane 0 of a row takes in the pointer phase: 4 h1[15] + c (scaled, frame constant and tag in c), in every lane
__device__ __forceinline__ uint32_t lin_hand_scaled_ror1(uint32_t h1, uint32_t v_c)
{
    uint32_t r;
    asm("v_pk_mad_u16 %0, %1, 4, %2 op_sel_hi:[1,0,1]\n\ts_nop 1\n\tv_mov_b32_dpp %0, %0" GACT_DPP_ROR1 : "=&v"(r) : "v"(h1), "v"(v_c));
    return r;
}
// lane n: h2[n - 1] - k2, lane 0 of a row: keeps first
__device__ __forceinline__ uint32_t lin_hand_shr1_over(uint32_t first, uint32_t h2, uint32_t v_k2)
{
    asm("s_nop 1\n\tv_sub_u32_dpp %0, %1, %2" GACT_DPP_SHR1 : "+v"(first) : "v"(h2), "v"(v_k2));
    return first;
}
// (a & ~b) | c in one fast-class instruction (v_bitop3_b32, gfx950; truth table over a = 0xF0, b = 0xCC, c = 0xAA)
template <bool BUILTIN = GACT_LIN_BUILTINS>
__device__ __forceinline__ uint32_t andn_or(uint32_t a, uint32_t b, uint32_t c)
{
    if constexpr (BUILTIN)
        return __builtin_amdgcn_bitop3_b32(a, b, c, 0xba);
    else {
        uint32_t r;
        asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xba" : "=v"(r) : "v"(a), "v"(b), "v"(c));
        return r;
    }
}
__device__ __forceinline__ uint32_t pk_ashr2(uint32_t a)
{
#if GACT_LIN_BUILTINS
    return __builtin_bit_cast(uint32_t, (LinS2)(__builtin_bit_cast(LinS2, a) >> (short)2));
#else
    uint32_t r;
    asm("v_pk_ashrrev_i16 %0, 2, %1 op_sel_hi:[0,1]" : "=v"(r) : "v"(a));
    return r;
#endif
}

// 8. Look-up words out of LDS (round 6).  A row's look-up word -- the one-hot byte table the v_perm of every column slot
//    reads -- used to be made per row and tile with a shift by the stream byte, a byte extraction and, in the pointer phase,
//    the +1 per byte: 8 of the 18 VALU instructions a step of the split pass spent outside its recurrence.  There are only
//    five such words per phase, so the block keeps them in LDS, [code 3, 2, 1, 0, pad] x [plain, pointer phase]
//    interleaved, and the stream byte (24 - 8 code, kLinPadRow for a row outside the tile) is the byte offset of the
//    pair: a ds_read_u8 and a ds_read_b32 with an immediate table address per row and tile, no VALU instruction.
//    word(b, plain) = dsub >> b, word(b, pointer phase) = (dsub4 >> b) + 0x01010101, the pad's 0 and 0x01010101.
//    (lin_lut_fill and LinLutLds: gact_p16.hpp, beside the loader that writes the stream)

// a selector of v_perm_b32 (a VOP3 instruction: no literal operand on gfx950) made where it is used.  As a plain constant
// the compiler hoists its s_mov_b32 out of every loop, the kernel's outermost one included, and the register is then held
// through the whole kernel: three of them cost the split kernel three more spilled SGPRs.
__device__ __forceinline__ uint32_t sconst_here(uint32_t lit)
{
    uint32_t r;
    asm volatile("s_mov_b32 %0, %1" : "=s"(r) : "i"(lit));
    return r;
}

// Pointer words of this pass (walk_chain's FMT 3): two bits per cell, the op code alone.  A half-word holds eight
// stored steps of one column (first step on top), a dword two adjacent columns (the even one low), a uint4 eight
// columns; a flush block is [uint4 n][lane], n < kUint4 (ws_quad_addr, gact_device.hpp).
template <int CW> struct LinWords {
    static constexpr int kWords = (CW + 1) / 2;          // dwords per lane, tile and flush
    static constexpr int kUint4 = (kWords + 3) / 4;
};
// acc[c]: the codes of column c, tile A in the low half-word, tile B in the high one.  storeA / storeB: does this lane
// write its words of tile A / tile B for this flush block (LinBand below: the block meets the band a walk can reach, or
// the tile stores everything)
template <int NW, int LANES, class Fix>
__device__ __forceinline__ void lin_flush(const uint32_t (&acc)[2 * NW], uint4 *qA, uint4 *qB, Fix fix, const bool storeA, const bool storeB)
{
    constexpr int QD = (NW + 3) / 4;
    uint32_t wa[QD * 4], wb[QD * 4];
#pragma unroll
    for (int n = 0; n < QD * 4; n++) {
        wa[n] = n < NW ? fix(__builtin_amdgcn_perm(acc[n < NW ? 2 * n + 1 : 0], acc[n < NW ? 2 * n : 0], 0x05040100u)) : 0u;
        wb[n] = n < NW ? fix(__builtin_amdgcn_perm(acc[n < NW ? 2 * n + 1 : 0], acc[n < NW ? 2 * n : 0], 0x07060302u)) : 0u;
    }
    if (storeA) {
#pragma unroll
        for (int q = 0; q < QD; q++) qA[q * kWsRow] = make_uint4(wa[4 * q], wa[4 * q + 1], wa[4 * q + 2], wa[4 * q + 3]);
    }
    if (storeB) {
#pragma unroll
        for (int q = 0; q < QD; q++) qB[q * kWsRow] = make_uint4(wb[4 * q], wb[4 * q + 1], wb[4 * q + 2], wb[4 * q + 3]);
    }
}

// 9. Byte groups (round 7).  Inside a whole flush block of the split pass a step's place in the block is a compile-time
//    fact, and filing a slot's 2-bit code -- a v_and_b32 and a v_pk_mad_u16 per slot and step -- is done for two columns
//    at once: one v_perm_b32 gathers the low bytes of a pair's two H'' (kLinPairSel: column c tile A, column c + 1 tile A,
//    column c tile B, column c + 1 tile B), one v_and_b32 cleans the four tags, and a byte takes four steps (first on top;
//    it starts empty and is shifted three times by two bits, so it never reaches its neighbour).  A block keeps two such
//    registers per pair, steps 0-3 and steps 4-7; the first step of each is a plain copy.  The flush builds LinWords'
//    dwords from them with one v_perm_b32 per pair and tile.  The slot without a partner keeps its half-word.
template <int S> struct LinPos { static constexpr int value = S; };       // a step's place in its block; kLinTail: in none
constexpr int kLinTail = -1;
constexpr uint32_t kLinPairSel = 0x06020400u;        // perm(H''[c + 1], H''[c], .)
constexpr uint32_t kLinPairMask = 0x03030303u;
constexpr uint32_t kLinFlushSelA = 0x05010400u;      // perm(steps 0-3, steps 4-7, .): {c + 1: 0-3, c + 1: 4-7, c: 0-3, c: 4-7} of tile A
constexpr uint32_t kLinFlushSelB = 0x07030602u;      // the same of tile B
// grp[2 p], grp[2 p + 1]: steps 0-3 and 4-7 of the pair of columns 2 p, 2 p + 1; odd: the half-words of column 2 NP (CW odd)
template <int CW>
__device__ __forceinline__ void lin_flush_groups(const uint32_t (&grp)[2 * (CW / 2)], const uint32_t odd, uint4 *qA, uint4 *qB,
                                                 const bool storeA, const bool storeB)
{
    constexpr int NP = CW / 2, NW = LinWords<CW>::kWords, QD = LinWords<CW>::kUint4;
    uint32_t wa[QD * 4], wb[QD * 4];
    const uint32_t sA = sconst_here(kLinFlushSelA), sB = sconst_here(kLinFlushSelB);
#pragma unroll
    for (int n = 0; n < QD * 4; n++) {
        wa[n] = n < NP ? __builtin_amdgcn_perm(grp[n < NP ? 2 * n : 0], grp[n < NP ? 2 * n + 1 : 0], sA)
              : n < NW ? odd & 0xffffu : 0u;
        wb[n] = n < NP ? __builtin_amdgcn_perm(grp[n < NP ? 2 * n : 0], grp[n < NP ? 2 * n + 1 : 0], sB)
              : n < NW ? odd >> 16 : 0u;
    }
    if (storeA) {
#pragma unroll
        for (int q = 0; q < QD; q++) qA[q * kWsRow] = make_uint4(wa[4 * q], wa[4 * q + 1], wa[4 * q + 2], wa[4 * q + 3]);
    }
    if (storeB) {
#pragma unroll
        for (int q = 0; q < QD; q++) qB[q * kWsRow] = make_uint4(wb[4 * q], wb[4 * q + 1], wb[4 * q + 2], wb[4 * q + 3]);
    }
}

// 6. Banded pointer stores (round 4).  A non-first tile's traceback starts at (R, Q) and moves up and to the left
//    (align.cpp:205-229); with di = R - i and dj = Q - j every move changes di - dj by at most one, and at the error rates
//    this aligner is made for the path stays within a few tens of columns of the diagonal di == dj for all of its <= 2 x early
//    steps.  The pass therefore stores, per lane, only the flush blocks that hold a cell with |di - dj| <= band -- about a
//    third of the window's 14 KB per tile -- and the walker checks at every region refill that it is still at least a
//    refill's worth of steps inside the band (walk_chain_lin, gact_chain.hpp).  A walk that is not gives up; its tile is run
//    again with every block stored (ChainState::full), the one case in some hundreds: exact by construction, whatever the
//    reads look like.  Every tile of a wave ends on the wave's last step (kEndAligned), so a cell's step is
//    T_end - di - (lanes between its lane and the lane of column Q): lane by lane a range of steps, [lo, hi].
constexpr int kLinBandDefault = 48, kLinBandMin = 24, kLinBandQuantum = 1;
struct LinBand {
    int lo[2], hi[2];          // steps whose cells of this lane lie inside the band, tile A / tile B (lo > hi: none)
    bool full[2];              // the tile stores every block of the window
    __device__ __forceinline__ bool store(int h, int first, int last) const { return full[h] | ((last >= lo[h]) & (first <= hi[h])); }
};
// lane's columns are dj_min .. dj_max away from column Q (dj_max < 0: pads right of the tile), `behind` lanes before Q's
__device__ __forceinline__ void lin_band_range(LinBand &b, int h, int T_end, int behind, int dj_min, int dj_max, int band, bool full)
{
    b.full[h] = full | (band <= 0);
    b.lo[h] = T_end - behind - dj_max - band;
    b.hi[h] = dj_max < 0 ? -0x40000000 : T_end - behind - imax(dj_min, 0) + band;
}

// ---------------------------------------------------------------------------
// Split layout (see gact_p16s.hpp for the column map).  Returns, in lane 15 of every group, H[R][Q] of both tiles
// (packed, plain scores) -- valid when every tile's last row is the wave's last step (shift = T_end - Tend).
template <int C1, int C2>
__device__ __forceinline__ uint32_t dp_pass_lin_split(const P16Consts &kc, const int gl,
                                                      const uint16_t *__restrict__ ref16,
                                                      const uint32_t (&qb)[C1 + C2],
                                                      const int T_end, const int tB,
                                                      uint32_t *__restrict__ wsA, uint32_t *__restrict__ wsB,
                                                      const int band, const bool fullA, const bool fullB,
                                                      const uint32_t *lut_lds)
{
    constexpr int CT = C1 + C2;
    constexpr int NW = LinWords<C2>::kWords, QD = LinWords<C2>::kUint4;
    constexpr int LAG = kGroup;
    const int g = (int)(int16_t)(kc.ext & 0xffffu);
    const uint32_t gv = vconst(kc.next), g4v = vconst(kc.next4), c3v = vconst(kc.c3), onev = vconst(kc.one),
                   dtv = vconst(kc.next4 + kc.tag1),               // 4|g| + 1: G'' (tagged 2) -> D'' tagged 1
                   c2v = vconst(kc.tag2);
    const uint32_t psel = sconst_here(kLinPairSel);
    // zero level of the row a lane did "before step 1": region 1 is at row t - gl, region 2 at row t - gl - LAG
    uint32_t Z1 = pk2(lin_base(g) + gl * g), Z2 = pk2(lin_base(g) + (gl + LAG) * g);
    uint32_t G[CT];                         // H of the previous row (drifted)
    uint32_t acc[2 * NW];                   // op codes of the last (up to) seven steps, one column each: the steps behind the last whole block
    uint32_t grp[2 * (C2 / 2)], odd = 0;    // op codes of a whole block, two columns each (9. above); nothing reads them before the
                                            // block's first step has written them
#pragma unroll
    for (int c = 0; c < CT; c++) G[c] = c < C1 ? Z1 : Z2;                          // row 0: H = 0
#pragma unroll
    for (int c = 0; c < 2 * NW; c++) acc[c] = 0;
    // last slot of each region as the neighbour lane will see it; on the j = 0 border it is the zero level
    uint32_t H1 = Z1, H2 = Z2;
    uint32_t Hdiag1 = Z1, Hdiag2 = Z2;

    // Look-up words (LinLut above): a row's byte in the ref stream IS the byte offset of its word in the table, so a row
    // costs two LDS reads per tile and no VALU instruction.  rp: this lane's stream bytes of region 2's row at the step
    // to come (tile A, tile B); region 1's are LAG entries further on.  Before step t: rb1 / rb1b = row t of region 1,
    // rb2 / rb2b = row t - LAG of region 2.
    typedef __attribute__((address_space(3))) const uint8_t LdsByte;
    typedef __attribute__((address_space(3))) const uint32_t LdsWord;
    LdsByte *const lut_plain = (LdsByte *)lut_lds, *const lut_tagged = (LdsByte *)(lut_lds + 1);
    auto row = [](LdsByte *table, uint32_t stream_byte) { return *(LdsWord *)(table + stream_byte); };
    LdsByte *rp = (LdsByte *)(ref16 + (1 - LAG));
    uint32_t rb1 = row(lut_plain, rp[2 * LAG]), rb1b = row(lut_plain, rp[2 * LAG + 1]);
    uint32_t rb2 = row(lut_plain, rp[0]), rb2b = row(lut_plain, rp[1]);
    rp += 2;

    // Instruction order.  With three waves on a SIMD a v_add / v_sub / v_and / v_or issues in 1.9 cycles when it does
    // not wait for the instruction in front of it, in 3.0 when it does (issue_rate_probe.json, dependent streams).
    // So the step is written in stages -- one kind of instruction for all column slots, then the next kind -- and the
    // two regions' column chains (H_left -> D -> H, two dependent instructions per slot) run side by side; the
    // scheduling barriers keep the compiler from folding the stages back into per-slot sequences.
#define GACT_SB() __builtin_amdgcn_sched_barrier(0)
    // the next step's rows: the stream bytes are asked for when the step begins, their look-up words once the v_perm stage
    // has read the current ones (the bytes have had that stage's time to arrive, the words have the rest of the step)
    uint32_t sb1 = 0, sb1b = 0, sb2 = 0, sb2b = 0;
    auto ask_bytes = [&](const bool r1, const bool r2) {
        if (r2) { sb2 = rp[0]; sb2b = rp[1]; }
        if (r1) { sb1 = rp[2 * LAG]; sb1b = rp[2 * LAG + 1]; }
        rp += 2;
    };
    auto ask_rows = [&](const bool r1, const bool r2, const bool tag2) {
        if (r1) { rb1 = row(lut_plain, sb1); rb1b = row(lut_plain, sb1b); }
        if (r2) { rb2 = row(tag2 ? lut_tagged : lut_plain, sb2); rb2b = row(tag2 ? lut_tagged : lut_plain, sb2b); }
    };
    auto upper_all = [&](auto first, uint32_t (&U)[CT], const bool tag2, const uint32_t Zr2) {
        constexpr int C0 = decltype(first)::value;
        uint32_t P[CT];
#pragma unroll
        for (int c = C0; c < CT; c++) P[c] = __builtin_amdgcn_perm(c < C1 ? rb1b : rb2b, c < C1 ? rb1 : rb2, qb[c]);
        GACT_SB();
#pragma unroll
        for (int c = C0; c < CT; c++) U[c] = (c == 0 ? Hdiag1 : c == C1 ? Hdiag2 : G[c - 1]) + P[c];   // align.cpp:134-144
        // (pointer phase: region 2's G is kept tagged 2, so it IS H_up'' as it stands; the look-up words of that phase
        //  carry a +1, so M'' = G_diag'' + 4 (sub - g) + 1 comes out tagged 3 with no instruction of its own)
        ask_rows(C0 == 0, true, tag2);
        GACT_SB();
        if (GACT_LIN_MAX3) {
#pragma unroll
            for (int c = C0; c < CT; c++)                                         // :145-147 and the insertion, :149-154
                U[c] = pk_max3f(U[c], c < C1 ? Z1 : Zr2, G[c]);
        } else {
#pragma unroll
            for (int c = C0; c < CT; c++) U[c] = lin_max(U[c], c < C1 ? Z1 : Zr2);     // :145-147
            GACT_SB();
#pragma unroll
            for (int c = C0; c < CT; c++) U[c] = lin_max(U[c], G[c]);              // the insertion, :149-154
        }
        GACT_SB();
    };

    auto step = [&]() {
        ask_bytes(true, true);
        Z1 += gv; Z2 += gv;
        // lane 0 of region 1 sits on the j = 0 border: the zero level
        const uint32_t Hl1 = (uint32_t)dpp_row_shr1((int)H1, (int)Z1);
        // lane 0 of region 2 continues lane 15's region 1 (one step ago = same row, same zero level)
        const uint32_t Hl2 = (uint32_t)dpp_row_shr1((int)H2, dpp_row_ror1((int)H1));
        uint32_t U[CT];
        upper_all(LinPos<0>{}, U, false, Z2);
        Hdiag1 = Hl1; Hdiag2 = Hl2;
        uint32_t Ha = Hl1, Hb = Hl2;
        static_assert(C2 >= C1, "region 2 is the longer chain");
#pragma unroll
        for (int c = 0; c < C1; c++) {                                           // :151-160 (no borrow)
            const uint32_t Da = Ha - gv, Db = Hb - gv;
            GACT_SB();
            G[c] = lin_max(U[c], Da); G[C1 + c] = lin_max(U[C1 + c], Db);
            GACT_SB();
            Ha = G[c]; Hb = G[C1 + c];
        }
#pragma unroll
        for (int c = 2 * C1; c < CT; c++) { G[c] = lin_max(U[c], Hb - gv); Hb = G[c]; }
        H1 = Ha; H2 = Hb;
    };
    // a step in which region 2 is in front of its row 1 in every lane (see 7. below): region 1 alone, region 2's zero level
    auto step_r1 = [&]() {
        ask_bytes(true, false);
        Z1 += gv; Z2 += gv;
        const uint32_t Hl1 = (uint32_t)dpp_row_shr1((int)H1, (int)Z1);
        uint32_t P[C1], U[C1];
#pragma unroll
        for (int c = 0; c < C1; c++) P[c] = __builtin_amdgcn_perm(rb1b, rb1, qb[c]);
        GACT_SB();
#pragma unroll
        for (int c = 0; c < C1; c++) U[c] = (c == 0 ? Hdiag1 : G[c - 1]) + P[c];
        ask_rows(true, false, false);
        GACT_SB();
#pragma unroll
        for (int c = 0; c < C1; c++) U[c] = GACT_LIN_MAX3 ? pk_max3f(U[c], Z1, G[c]) : lin_max(lin_max(U[c], Z1), G[c]);
        GACT_SB();
        Hdiag1 = Hl1;
        uint32_t Ha = Hl1;
#pragma unroll
        for (int c = 0; c < C1; c++) { G[c] = lin_max(U[c], Ha - gv); Ha = G[c]; }
        H1 = Ha;
    };

    // ---- pointer phase: region 2 on tagged scores; G = 4H + 2 there: H_up'' without an instruction, the diagonal gets
    //      its tag 3 from the look-up word (+1), the left neighbour its tag 1 from the gap subtraction (4|g| + 1), and
    //      "low bits := 2" is one fast-class v_bitop3_b32
    uint32_t Z24 = 0;
    // filing the codes.  A step of the remainder (kLinTail): slot c's code goes into acc[c], a v_and_b32 beside the v_bitop3 and a
    // v_pk_mad_u16 beside the next slot's maximum.  Step S of a whole block: the pair's v_perm_b32 stands where the odd column's
    // v_and_b32 stood, its v_and_b32 beside the next slot's subtraction, its v_pk_mad_u16 (none at S = 0 and S = 4) beside
    // that slot's maximum; Hq: the even column's H'' until its partner's exists
    static_assert(C2 >= 3 && (C2 & 1), "the last pair is filed while the unpaired slot is computed");
    auto file_group = [&](const int S, const int c, const uint32_t x) {
        uint32_t &r = grp[c - 2 + (S >> 2)];
        r = (S & 3) ? pk_shl_add4(r, x) : x;
    };
    auto step_ptr = [&](auto pos, auto with_r1) {
        constexpr int S = decltype(pos)::value;
        constexpr bool blk = S != kLinTail;
        constexpr bool R1 = decltype(with_r1)::value;
        ask_bytes(R1, true);
        if (R1) Z1 += gv;
        Z24 += g4v;
        uint32_t Hl1 = 0;
        if (R1) Hl1 = (uint32_t)dpp_row_shr1((int)H1, (int)Z1);
        const uint32_t Hl2 = (uint32_t)dpp_row_shr1((int)H2, dpp_row_ror1((int)pk_mad4v(H1, c2v)));
        uint32_t U[CT];
        upper_all(LinPos<R1 ? 0 : C1>{}, U, true, Z24);
        if (R1) Hdiag1 = Hl1;
        Hdiag2 = Hl2;
        uint32_t Ha = Hl1, Hb = Hl2;
        uint32_t tprev = 0, Hq = 0, x = 0;
#pragma unroll
        for (int c = 0; c < C2; c++) {
            const bool both = R1 && c < C1;
            const bool filed = blk && c >= 2 && !(c & 1);
            uint32_t Da = 0;
            const uint32_t Db = Hb - dtv;
            if (both) Da = Ha - gv;
            if (filed) x &= kLinPairMask;
            GACT_SB();
            const uint32_t Hp = lin_max(U[C1 + c], Db);
            if (both) { G[c] = lin_max(U[c], Da); Ha = G[c]; }
            if (!blk && c > 0) acc[c - 1] = pk_shl_add4(acc[c - 1], tprev);
            if (filed) file_group(S, c, x);
            GACT_SB();
            G[C1 + c] = andn_or(Hp, c3v, c2v);
            if (!blk || c == C2 - 1) tprev = Hp & c3v;
            else if (c & 1) x = __builtin_amdgcn_perm(Hp, Hq, psel);
            else Hq = Hp;
            GACT_SB();
            Hb = G[C1 + c];
        }
        if (!blk) acc[C2 - 1] = pk_shl_add4(acc[C2 - 1], tprev);
        else odd = S ? pk_shl_add4(odd, tprev) : tprev;
        if (R1) H1 = Ha;
        H2 = Hb;
    };
    auto step_tagged = [&](auto pos) { step_ptr(pos, std::true_type{}); };
    auto step_tagged_r2 = [&](auto pos) { step_ptr(pos, std::false_type{}); };
    // the eight steps of a whole block, each with its place
#define GACT_LIN_BLOCK8(f) do { f(LinPos<0>{}); f(LinPos<1>{}); f(LinPos<2>{}); f(LinPos<3>{}); \
                                f(LinPos<4>{}); f(LinPos<5>{}); f(LinPos<6>{}); f(LinPos<7>{}); } while (0)
    auto enter_tagged = [&]() {
#pragma unroll
        for (int c = C1; c < CT; c++) G[c] = pk_mad4v(G[c], c2v);
        H2 = pk_mad4v(H2, c2v);
        Hdiag2 = pk_mad4v(Hdiag2, c2v);
        Z24 = pk_mad4v(Z2, c3v);                        // the zero level stays tagged 3 (H == 0 reads as MATCH, see 3.)
        // the row already fetched, from the pointer phase's table: bonus times four, + 1
        rb2 = row(lut_tagged, rp[-2]); rb2b = row(lut_tagged, rp[-1]);
    };

    int t = 1;
    // 7. Region 2 runs LAG steps behind region 1 and every tile ends on the wave's last step: for the first LAG steps region 2
    //    is in front of its row 1 in EVERY lane (its values are the zero level, whatever the reads hold), for the last LAG
    //    steps region 1 is past its last row in every lane (nothing reads what it would compute: lane 0 of region 2 takes
    //    lane 15's H of step T_end - LAG at step T_end - LAG + 1 and rows past R after that).  Those steps run without the
    //    idle region's column slots: 16 x 65 + up to 16 x 37 of a pass's ~53 k instructions.
    for (const int tP = imin(LAG, imin(tB - 1, T_end)); t <= tP; t++) step_r1();
    if (t > 1) {
#pragma unroll
        for (int c = C1; c < CT; c++) G[c] = Z2;
        H2 = Z2; Hdiag2 = Z2;
        rb2 = row(lut_plain, rp[-2]); rb2b = row(lut_plain, rp[-1]);
    }
    // (two steps per trip: the hand-over of the diagonal's registers from step to step is then a renaming)
    const int tU = imin(tB - 1, T_end);
    for (; t + 1 <= tU; t += 2) { step(); step(); }
    if (t <= tU) { step(); t++; }
    const bool tagged = t <= T_end;
    if (tagged) enter_tagged();
    uint4 *qA = reinterpret_cast<uint4 *>(wsA) + gl;
    uint4 *qB = reinterpret_cast<uint4 *>(wsB) + gl;
    // region 2 is right-aligned: lane gl's columns are 13 (15 - gl) .. 13 (15 - gl) + 12 away from column Q in EVERY tile
    // (quantum: lanes store in aligned groups of 1, 4 or 8 -- whole 64- or 128-byte pieces of a workspace row -- so that the
    //  walker's loads never meet a partly written cache line; both ends of a lane's range grow with the lane)
    LinBand bd;
    {
        const int q1 = (band >> 16) - 1, b = band & 0xffff;
        const int u_lo = kGroup - 1 - (gl & ~q1), u_hi = kGroup - 1 - (gl | q1);
        LinBand lo_, hi_;
        lin_band_range(lo_, 0, T_end, u_lo, C2 * u_lo, C2 * u_lo + C2 - 1, b, fullA);
        lin_band_range(hi_, 0, T_end, u_hi, C2 * u_hi, C2 * u_hi + C2 - 1, b, fullA);
        bd.lo[0] = bd.lo[1] = lo_.lo[0]; bd.hi[0] = bd.hi[1] = hi_.hi[0];
        bd.full[0] = fullA | (b <= 0); bd.full[1] = fullB | (b <= 0);
    }
    // whole blocks of eight steps, each followed by its flush (an `if ((k & 7) == 7)` inside one loop is
    // if-converted by the compiler: the re-pairing v_perm of the flush would then run at every step)
    int k = 0;
    // (two loops one behind the other, not one loop with a branch inside: the two kinds of step keep their registers
    //  differently, and a loop that holds both moves ~90 registers per block to reconcile them)
    // (the eight steps are straight-line code: the stream offsets are immediates, the diagonal's registers are renamed)
    // (a whole block keeps its codes in the byte groups and leaves acc[] alone: zero, as the remainder's partial flush needs it)
    while (t + 7 <= T_end && t <= T_end - LAG) {
        GACT_LIN_BLOCK8(step_tagged);
        t += 8; k += 8;
        lin_flush_groups<C2>(grp, odd, qA, qB, bd.store(0, t - 8, t - 1), bd.store(1, t - 8, t - 1));
        qA += QD * kWsRow;
        qB += QD * kWsRow;
    }
    while (t + 7 <= T_end) {
        GACT_LIN_BLOCK8(step_tagged_r2);
        t += 8; k += 8;
        lin_flush_groups<C2>(grp, odd, qA, qB, bd.store(0, t - 8, t - 1), bd.store(1, t - 8, t - 1));
        qA += QD * kWsRow;
        qB += QD * kWsRow;
    }
    // (what is left are the last seven steps at most: region 2 alone, unless the pointer phase began inside them)
    for (; t <= T_end - LAG; t++, k++) step_tagged(LinPos<kLinTail>{});
    for (; t <= T_end; t++, k++) step_tagged_r2(LinPos<kLinTail>{});
    if (k & 7) {
        const int sh = 2 * (8 - (k & 7));
        lin_flush<NW, kGroup>(acc, qA, qB, [sh](uint32_t w) { return ((w & 0xffffu) << sh & 0xffffu) | ((w >> 16) << sh << 16); },
                              bd.store(0, t - (k & 7), t - 1), bd.store(1, t - (k & 7), t - 1));
    }
    // H of the last column at the row of the last step, drift taken off
    return tagged ? pk_ashr2(lin_sub(H2 | kc.c3, Z24)) : lin_sub(H2, Z2);
}

// 13. Sliding the zero levels (round 10; GACT_LIN_SLIDE=0 builds the per-step additions of 2b.).  The zero level of step t
//     and slot c is Zw(t + c): from one step to the next the window does not change its contents, it moves up by one entry.
//     Inside a block of kLinBlock steps whose places are compile-time facts (LinPos) the pass therefore keeps a STRIP of
//     levels that covers the whole block, strip[j] = Zw(t0 - 1 + j) with t0 the block's first step (4 Zw(t0 + j) + 3 for
//     the pointer phase's region 2), and step S reads strip[S + k] where the per-step form reads W[k] / T[k]: a renaming,
//     no instruction.  The strip moves once per block, by kLinBlock |g| per entry (lin_strip_slide: opaque s_add_u32, several
//     to an asm statement -- the hazard recogniser puts an s_nop behind a statement, not behind an instruction).
//     The per-step form (the remainders, step_r1) keeps W[k] = Zw(t - 2 + k) BEFORE step t and adds |g| when the step begins;
//     the strip holds the levels DURING the block's first step.  lin_strip_enter takes the first N entries from the one form
//     to the other and builds the entries above them; lin_strip_leave takes them back (the strip has moved behind the last
//     block, so its first N entries are then the levels during the step to come).  A handful of scalar instructions per
//     phase and pass.  tests/test_lin_level_window.py drives exactly these helpers through the pass's loop structure.
#ifndef GACT_LIN_SLIDE
#define GACT_LIN_SLIDE 1
#endif
constexpr int kLinBlock = 8;
// entries of a strip that serves a window of n levels through a block
__host__ __device__ constexpr int lin_strip_len(int n, int steps = kLinBlock) { return GACT_LIN_SLIDE ? n + steps - 1 : n; }
// the entry step S of a block reads for window entry k (a remainder step, or the per-step build: the window itself)
__host__ __device__ constexpr int lin_strip_at(int S, int k) { return GACT_LIN_SLIDE && S != kLinTail ? S + k : k; }
template <int N, int STEPS = kLinBlock, int LEN>
__host__ __device__ __forceinline__ void lin_strip_enter(uint32_t (&s)[LEN], const uint32_t by)
{
    static_assert(lin_strip_len(N, STEPS) <= LEN, "the strip fits its registers");
#pragma unroll
    for (int k = 0; k < N; k++) s[k] += by;
#pragma unroll
    for (int k = N; k < lin_strip_len(N, STEPS); k++) s[k] = s[k - 1] + by;
}
template <int N, int LEN>
__host__ __device__ __forceinline__ void lin_strip_leave(uint32_t (&s)[LEN], const uint32_t by)
{
#pragma unroll
    for (int k = 0; k < N; k++) s[k] -= by;
}
// behind a block: every entry up by kLinBlock steps' worth (by_block); add4 / add1: four additions, one
template <int N, int STEPS = kLinBlock, int LEN, class Add4, class Add1>
__host__ __device__ __forceinline__ void lin_strip_slide(uint32_t (&s)[LEN], const uint32_t by_block, Add4 add4, Add1 add1)
{
    constexpr int M = lin_strip_len(N, STEPS);
#pragma unroll
    for (int j = 0; j + 4 <= M; j += 4) add4(s[j], s[j + 1], s[j + 2], s[j + 3], by_block);
#pragma unroll
    for (int j = M & ~3; j < M; j++) add1(s[j], by_block);
}

// ---------------------------------------------------------------------------
// Split layout in the column-drifted frame (2b. above; which of the two runs: 12.): the same pass, same arguments.  Returns, in lane 15 of every group, H[R][Q] of both tiles
// (packed, plain scores) -- valid when every tile's last row is the wave's last step (shift = T_end - Tend).
template <int C1, int C2>
__device__ __forceinline__ uint32_t dp_pass_lin_split_col(const P16Consts &kc, const int gl,
                                                      const uint16_t *__restrict__ ref16,
                                                      const uint32_t (&qb)[C1 + C2],
                                                      const int T_end, const int tB,
                                                      uint32_t *__restrict__ wsA, uint32_t *__restrict__ wsB,
                                                      const int band, const bool fullA, const bool fullB,
                                                      const uint32_t *lut_lds)
{
    constexpr int CT = C1 + C2;
    constexpr int NW = LinWords<C2>::kWords, QD = LinWords<C2>::kUint4;
    constexpr int LAG = kGroup;
    const int g = (int)(int16_t)(kc.ext & 0xffffu);
    const uint32_t gs = kc.next, g4s = kc.next4;                       // |g|, 4|g|: what the windows move by per step
    const uint32_t k1v = vconst((uint32_t)(C1 - 1) * kc.next),         // hand-over between lanes of region 1: (C1 - 1)|g|
                   k2v = vconst((uint32_t)(C2 - 1) * kc.next);         // ... of region 2
    // the pointer phase's constants are made where it begins (enter_tagged): k2v's register is free by then
    uint32_t c3v = 0, onev = 0, c2v = 0,
             k24v = 0,                                                 // hand-over between lanes of region 2 on tagged scores
             k12v = 0;   // region 1 into region 2, scaled: 4 (H - (C1 - 1)|g|) + 2
    const uint32_t psel = sconst_here(kLinPairSel);
    // the zero levels (2b. above).  During step t W[k] = Zw(t - 1 + k): W[0] the j = 0 border, W[c + 1] slot c of either
    // region; in the pointer phase T[c] = 4 Zw(t + c) + 3 is region 2's.  Wave-uniform: SGPRs, moved by the scalar unit
    constexpr int NWIN = C2 + 1;
    // (GACT_LIN_SLIDE: strips, 13. above -- the window is their first NWIN / C1 + 1 / C2 entries between the block loops)
    uint32_t W[lin_strip_len(NWIN)], T[lin_strip_len(C2)];
#pragma unroll
    for (int k = 0; k < NWIN; k++) W[k] = pk2(lin_base(g) + (k - 1) * (-g));      // before step 1: Zw(k - 1)
#pragma unroll
    for (int c = 0; c < lin_strip_len(C2); c++) T[c] = 0;
#pragma unroll
    for (int k = NWIN; k < lin_strip_len(NWIN); k++) W[k] = 0;
    // (an opaque addition in the pointer phase, a plain one on plain scores: 12. above)
    auto bump = [](uint32_t &z, const uint32_t by) { asm("s_add_u32 %0, %0, %1" : "+s"(z) : "s"(by) : "scc"); };
    auto advance = [&](const int nW, const bool tagged_too) {
#pragma unroll
        for (int k = 0; k < NWIN; k++) if (k < nW) { if (tagged_too) bump(W[k], gs); else W[k] += gs; }
        if (tagged_too) {
#pragma unroll
            for (int c = 0; c < C2; c++) bump(T[c], g4s);
        }
    };
    auto bump4 = [](uint32_t &z0, uint32_t &z1, uint32_t &z2, uint32_t &z3, const uint32_t by) {
        asm("s_add_u32 %0, %0, %4\n\ts_add_u32 %1, %1, %4\n\ts_add_u32 %2, %2, %4\n\ts_add_u32 %3, %3, %4"
            : "+s"(z0), "+s"(z1), "+s"(z2), "+s"(z3) : "s"(by) : "scc");
    };
    uint32_t G[CT];                         // H of the previous row (drifted)
    uint32_t acc[2 * NW];                   // op codes of the last (up to) seven steps, one column each: the steps behind the last whole block
    uint32_t grp[2 * (C2 / 2)], odd = 0;    // op codes of a whole block, two columns each (9. above); nothing reads them before the
                                            // block's first step has written them
#pragma unroll
    for (int c = 0; c < CT; c++) G[c] = W[(c < C1 ? c : c - C1) + 1];             // row 0: H = 0, in the frame of "step 0"
#pragma unroll
    for (int c = 0; c < 2 * NW; c++) acc[c] = 0;
    // last slot of each region as the neighbour lane will see it; on the j = 0 border it is the zero level
    uint32_t H1 = W[C1], H2 = W[C2];
    uint32_t Hdiag1 = W[0], Hdiag2 = W[0];          // last step's hand-over value: one gap below the zero level of slot 0 then

    // look-up words and the ref stream: as in dp_pass_lin_split
    typedef __attribute__((address_space(3))) const uint8_t LdsByte;
    typedef __attribute__((address_space(3))) const uint32_t LdsWord;
    LdsByte *const lut_plain = (LdsByte *)lut_lds, *const lut_tagged = (LdsByte *)(lut_lds + 1);
    auto row = [](LdsByte *table, uint32_t stream_byte) { return *(LdsWord *)(table + stream_byte); };
    LdsByte *rp = (LdsByte *)(ref16 + (1 - LAG));
    uint32_t rb1 = row(lut_plain, rp[2 * LAG]), rb1b = row(lut_plain, rp[2 * LAG + 1]);
    uint32_t rb2 = row(lut_plain, rp[0]), rb2b = row(lut_plain, rp[1]);
    rp += 2;

    // (instruction order, and when the next step's rows are asked for: see dp_pass_lin_split)
    uint32_t sb1 = 0, sb1b = 0, sb2 = 0, sb2b = 0;
    auto ask_bytes = [&](const bool r1, const bool r2) {
        if (r2) { sb2 = rp[0]; sb2b = rp[1]; }
        if (r1) { sb1 = rp[2 * LAG]; sb1b = rp[2 * LAG + 1]; }
        rp += 2;
    };
    auto ask_rows = [&](const bool r1, const bool r2, const bool tag2) {
        if (r1) { rb1 = row(lut_plain, sb1); rb1b = row(lut_plain, sb1b); }
        if (r2) { rb2 = row(tag2 ? lut_tagged : lut_plain, sb2); rb2b = row(tag2 ? lut_tagged : lut_plain, sb2b); }
    };
    // slots first .. last - 1: both regions, or the one a step computes.  o: the step's place in a block's strips
    // (lin_strip_at), 0 for a step of the per-step form
    auto upper_all = [&](auto first, auto last, uint32_t (&U)[CT], const bool tag2, const int o) {
        constexpr int C0 = decltype(first)::value, Cn = decltype(last)::value;
        uint32_t P[CT];
#pragma unroll
        for (int c = C0; c < Cn; c++) P[c] = __builtin_amdgcn_perm(c < C1 ? rb1b : rb2b, c < C1 ? rb1 : rb2, qb[c]);
        GACT_SB();
#pragma unroll
        for (int c = C0; c < Cn; c++) U[c] = (c == 0 ? Hdiag1 : c == C1 ? Hdiag2 : G[c - 1]) + P[c];   // align.cpp:134-144
        ask_rows(C0 < C1, Cn > C1, tag2);
        GACT_SB();
        if (GACT_LIN_MAX3) {
#pragma unroll
            for (int c = C0; c < Cn; c++)                                        // :145-147 and the insertion, :149-154
                U[c] = pk_max3f_s(U[c], c < C1 ? W[o + c + 1] : tag2 ? T[o + c - C1] : W[o + c - C1 + 1], G[c]);
        } else {
#pragma unroll
            for (int c = C0; c < Cn; c++) U[c] = pk_max_sgpr(U[c], c < C1 ? W[o + c + 1] : tag2 ? T[o + c - C1] : W[o + c - C1 + 1]);     // :145-147
            GACT_SB();
#pragma unroll
            for (int c = C0; c < Cn; c++) U[c] = lin_max<kLinSplitBuiltins>(U[c], G[c]);             // the insertion, :149-154
        }
        GACT_SB();
    };

    // a step on plain scores.  Without region 2: it is in front of its row 1 in every lane (see 7. below) and stays at its
    // zero level
    auto step_plain = [&](auto pos, auto with_r2) {
        constexpr int S = decltype(pos)::value, o = lin_strip_at(S, 0);
        constexpr bool R2 = decltype(with_r2)::value;
        ask_bytes(true, R2);
        if (!GACT_LIN_SLIDE || S == kLinTail) advance(R2 ? NWIN : C1 + 1, false);
        // lane 0 of region 1 sits on the j = 0 border: one gap below its zero level
        const uint32_t Hl1 = lin_hand_shr1(H1, k1v, W[o]);
        // lane 0 of region 2 continues lane 15's region 1 (one step ago = same row)
        uint32_t Hl2 = 0;
        if (R2) Hl2 = lin_hand_ror1_shr1(H1, k1v, H2, k2v);
        uint32_t U[CT];
        upper_all(LinPos<0>{}, LinPos<R2 ? CT : C1>{}, U, false, o);
        Hdiag1 = Hl1;
        if (R2) Hdiag2 = Hl2;
        uint32_t Ha = Hl1, Hb = Hl2;
        static_assert(C2 >= C1, "region 2 is the longer chain");
#pragma unroll
        for (int c = 0; c < C1; c++) {                                           // :151-160: H_left + g is H_left as it stands
            G[c] = lin_max<kLinSplitBuiltins>(U[c], Ha);
            if (R2) { G[C1 + c] = lin_max<kLinSplitBuiltins>(U[C1 + c], Hb); GACT_SB(); Hb = G[C1 + c]; }
            Ha = G[c];
        }
        H1 = Ha;
        if (R2) {
#pragma unroll
            for (int c = 2 * C1; c < CT; c++) { G[c] = lin_max<kLinSplitBuiltins>(U[c], Hb); Hb = G[c]; }
            H2 = Hb;
        }
    };
    auto step = [&](auto pos) { step_plain(pos, std::true_type{}); };
    auto step_r1 = [&]() { step_plain(LinPos<kLinTail>{}, std::false_type{}); };

    // ---- pointer phase and the filing of the codes: as in dp_pass_lin_split; what is left of the left neighbour's gap
    //      subtraction is the re-tag 2 -> 1, a - 1
    static_assert(C2 >= 3 && (C2 & 1), "the last pair is filed while the unpaired slot is computed");
    auto file_group = [&](const int S, const int c, const uint32_t x) {
        uint32_t &r = grp[c - 2 + (S >> 2)];
        r = (S & 3) ? pk_shl_add4(r, x) : x;
    };
    // a step of the pointer phase.  Without region 1: it is past its last row in every lane (see 7. below); H1 stays what
    // lane 15 left at step T_end - LAG
    auto step_ptr = [&](auto pos, auto with_r1) {
        constexpr int S = decltype(pos)::value;
        constexpr bool blk = S != kLinTail;
        constexpr bool R1 = decltype(with_r1)::value;
        constexpr int o = lin_strip_at(S, 0);
        ask_bytes(R1, true);
        if (!GACT_LIN_SLIDE || !blk) advance(R1 ? C1 + 1 : 0, true);
        uint32_t Hl1 = 0;
        if (R1) Hl1 = lin_hand_shr1(H1, k1v, W[o]);
        // lane 15's region-1 column enters region 2 scaled and tagged 2
        const uint32_t Hl2 = lin_hand_shr1_over(lin_hand_scaled_ror1(H1, k12v), H2, k24v);
        uint32_t U[CT];
        upper_all(LinPos<R1 ? 0 : C1>{}, LinPos<CT>{}, U, true, o);
        if (R1) Hdiag1 = Hl1;
        Hdiag2 = Hl2;
        uint32_t Ha = Hl1, Hb = Hl2;
        uint32_t tprev = 0, Hq = 0, x = 0;
#pragma unroll
        for (int c = 0; c < C2; c++) {
            const bool both = R1 && c < C1;
            const bool filed = blk && c >= 2 && !(c & 1);                        // the pair (c - 2, c - 1) is filed in this slot
            const uint32_t Db = Hb - onev;                                       // G'' tagged 2 -> D'' tagged 1
            if (filed) x &= kLinPairMask;
            GACT_SB();
            const uint32_t Hp = lin_max<kLinSplitBuiltins>(U[C1 + c], Db);       // the low bits: the op (:162-164)
            if (both) { G[c] = lin_max<kLinSplitBuiltins>(U[c], Ha); Ha = G[c]; }
            if (!blk && c > 0) acc[c - 1] = pk_shl_add4(acc[c - 1], tprev);
            if (filed) file_group(S, c, x);
            GACT_SB();
            G[C1 + c] = andn_or<kLinSplitBuiltins>(Hp, c3v, c2v);                // low bits := 2
            if (!blk || c == C2 - 1) tprev = Hp & c3v;
            else if (c & 1) x = __builtin_amdgcn_perm(Hp, Hq, psel);
            else Hq = Hp;
            GACT_SB();
            Hb = G[C1 + c];
        }
        if (!blk) acc[C2 - 1] = pk_shl_add4(acc[C2 - 1], tprev);
        else odd = S ? pk_shl_add4(odd, tprev) : tprev;
        if (R1) H1 = Ha;
        H2 = Hb;
    };
    auto step_tagged = [&](auto pos) { step_ptr(pos, std::true_type{}); };
    auto step_tagged_r2 = [&](auto pos) { step_ptr(pos, std::false_type{}); };
    // the eight steps of a whole block, each with its place
#undef GACT_SB
    auto enter_tagged = [&]() {
        c3v = vconst(kc.c3); onev = vconst(kc.one); c2v = vconst(kc.tag2);
        k24v = vconst((uint32_t)(C2 - 1) * kc.next4);
        k12v = vconst(pk2(2 + 4 * (C1 - 1) * g));
#pragma unroll
        for (int c = C1; c < CT; c++) G[c] = pk_mad4v(G[c], c2v);
        H2 = pk_mad4v(H2, c2v);
        Hdiag2 = pk_mad4v(Hdiag2, c2v);
#pragma unroll
        for (int c = 0; c < C2; c++) T[c] = (W[c + 1] << 2) + kc.c3;   // the zero levels stay tagged 3 (H == 0 reads as MATCH, see 3.)
        // the row already fetched, from the pointer phase's table: bonus times four, + 1
        rb2 = row(lut_tagged, rp[-2]); rb2b = row(lut_tagged, rp[-1]);
    };

    int t = 1;
    // (7. in dp_pass_lin_split: the first and the last LAG steps run without the idle region's column slots)
    for (const int tP = imin(LAG, imin(tB - 1, T_end)); t <= tP; t++) step_r1();
    if (t > 1) {
        // region 2 starts at its zero level: what its slots "computed" at step t - 1, in that step's frame
#pragma unroll
        for (int k = C1 + 1; k < NWIN; k++) W[k] = W[k - 1] + gs;
#pragma unroll
        for (int c = C1; c < CT; c++) G[c] = W[c - C1 + 1];
        H2 = W[C2]; Hdiag2 = W[0];
        rb2 = row(lut_plain, rp[-2]); rb2b = row(lut_plain, rp[-1]);
    }
    // (two steps per trip: the hand-over of the diagonal's registers from step to step is then a renaming)
    const int tU = imin(tB - 1, T_end);
#if GACT_LIN_SLIDE
    // (13. above: eight steps per trip on a strip of NWIN + 7 levels; the steps left over in the two-step form below --
    //  as a single-step loop they cost the cooperative kernel two more spilled VGPRs)
    lin_strip_enter<NWIN>(W, gs);
    for (; t + kLinBlock - 1 <= tU; t += kLinBlock) {
        GACT_LIN_BLOCK8(step);
        lin_strip_slide<NWIN>(W, gs * kLinBlock, bump4, bump);
    }
    lin_strip_leave<NWIN>(W, gs);
#endif
    for (; t + 1 <= tU; t += 2) { step(LinPos<kLinTail>{}); step(LinPos<kLinTail>{}); }
    if (t <= tU) { step(LinPos<kLinTail>{}); t++; }
    const bool tagged = t <= T_end;
    if (tagged) enter_tagged();
    uint4 *qA = reinterpret_cast<uint4 *>(wsA) + gl;
    uint4 *qB = reinterpret_cast<uint4 *>(wsB) + gl;
    // region 2 is right-aligned: lane gl's columns are 13 (15 - gl) .. 13 (15 - gl) + 12 away from column Q in EVERY tile
    // (quantum: lanes store in aligned groups of 1, 4 or 8 -- whole 64- or 128-byte pieces of a workspace row -- so that the
    //  walker's loads never meet a partly written cache line; both ends of a lane's range grow with the lane)
    LinBand bd;
    {
        const int q1 = (band >> 16) - 1, b = band & 0xffff;
        const int u_lo = kGroup - 1 - (gl & ~q1), u_hi = kGroup - 1 - (gl | q1);
        LinBand lo_, hi_;
        lin_band_range(lo_, 0, T_end, u_lo, C2 * u_lo, C2 * u_lo + C2 - 1, b, fullA);
        lin_band_range(hi_, 0, T_end, u_hi, C2 * u_hi, C2 * u_hi + C2 - 1, b, fullA);
        bd.lo[0] = bd.lo[1] = lo_.lo[0]; bd.hi[0] = bd.hi[1] = hi_.hi[0];
        bd.full[0] = fullA | (b <= 0); bd.full[1] = fullB | (b <= 0);
    }
    // whole blocks of eight steps, each followed by its flush
    int k = 0;
#if GACT_LIN_SLIDE
    // (13. above: region 1's and the border's C1 + 1 levels and region 2's C2 scaled ones become strips for the whole blocks)
    if (tagged) { lin_strip_enter<C1 + 1>(W, gs); lin_strip_enter<C2>(T, g4s); }
#endif
    // (two loops, straight-line steps, acc[] left alone: the notes at the same place in dp_pass_lin_split)
    while (t + 7 <= T_end && t <= T_end - LAG) {
        GACT_LIN_BLOCK8(step_tagged);
        t += 8; k += 8;
#if GACT_LIN_SLIDE
        lin_strip_slide<C1 + 1>(W, gs * kLinBlock, bump4, bump);
        lin_strip_slide<C2>(T, g4s * kLinBlock, bump4, bump);
#endif
        lin_flush_groups<C2>(grp, odd, qA, qB, bd.store(0, t - 8, t - 1), bd.store(1, t - 8, t - 1));
        qA += QD * kWsRow;
        qB += QD * kWsRow;
    }
    while (t + 7 <= T_end) {
        GACT_LIN_BLOCK8(step_tagged_r2);
        t += 8; k += 8;
#if GACT_LIN_SLIDE
        lin_strip_slide<C2>(T, g4s * kLinBlock, bump4, bump);
#endif
        lin_flush_groups<C2>(grp, odd, qA, qB, bd.store(0, t - 8, t - 1), bd.store(1, t - 8, t - 1));
        qA += QD * kWsRow;
        qB += QD * kWsRow;
    }
#undef GACT_LIN_BLOCK8
#if GACT_LIN_SLIDE
    if (tagged) { lin_strip_leave<C1 + 1>(W, gs); lin_strip_leave<C2>(T, g4s); }
#endif
    // (what is left are the last seven steps at most: region 2 alone, unless the pointer phase began inside them)
    for (; t <= T_end - LAG; t++, k++) step_tagged(LinPos<kLinTail>{});
    for (; t <= T_end; t++, k++) step_tagged_r2(LinPos<kLinTail>{});
    if (k & 7) {
        const int sh = 2 * (8 - (k & 7));
        lin_flush<NW, kGroup>(acc, qA, qB, [sh](uint32_t w) { return ((w & 0xffffu) << sh & 0xffffu) | ((w >> 16) << sh << 16); },
                              bd.store(0, t - (k & 7), t - 1), bd.store(1, t - (k & 7), t - 1));
    }
    // H of the last column at the row of the last step, drift taken off
    return tagged ? pk_ashr2(lin_sub(H2 | kc.c3, T[C2 - 1])) : lin_sub(H2, W[C2]);
}
#undef GACT_DPP_SHR1
#undef GACT_DPP_ROR1

// ---------------------------------------------------------------------------
// Uniform layout (lane gl owns columns gl*C .. gl*C + C-1; 16 or 32 lanes per tile pair), every slot tagged in the
// pointer phase.  Two users: the wide main launch (LANES = 32, few long chains) and, with AMAX, the seed launch
// (first tiles: pointers from step 1 on, arg-max of align.cpp:173-177 as in dp_pass_p16 -- the key 8H + (step & 7)
// is 2 G'' - 2 Z'' + (step & 7) on the scaled, drifted scores).
// Returns, in the lane of column Q_h, H[R][Q] of tile h in half-word h (cq[h] = that column's slot); valid when
// every tile's last row is the wave's last step.  AMAX: the return value is not used (the walk starts at the
// arg-max with its score).
template <int C, int LANES, bool AMAX>
__device__ __forceinline__ uint32_t dp_pass_lin(const P16Consts &kc, const int gl,
                                                const uint16_t *__restrict__ ref16,
                                                const uint32_t (&qb)[C],
                                                const int T_end, const int tB,
                                                uint32_t *__restrict__ wsA, uint32_t *__restrict__ wsB,
                                                const int cqA, const int cqB, const int (*RQ)[2], P16Best *pb,
                                                const int col_from, const int band, const int QA, const int QB,
                                                const bool fullA, const bool fullB)
{
    constexpr int NW = LinWords<C>::kWords, QD = LinWords<C>::kUint4;
    // col_from: first column (1-based) a walk can reach in either tile: lanes left of it keep their words
    const bool store = AMAX || gl * C + C >= col_from;
    // band (non-first tiles, see LinBand): the lane's columns gl C + 1 .. gl C + C are Q - gl C - C .. Q - gl C - 1 away from
    // column Q, whose lane is (Q - 1) / C
    LinBand bd;
    {
        const int q1 = AMAX ? 0 : (band >> 16) - 1, b = AMAX ? 0 : band & 0xffff;     // (quantum: see dp_pass_lin_split)
        const int g_lo = gl & ~q1, g_hi = gl | q1;
        LinBand lo_, hi_;
        lin_band_range(lo_, 0, T_end, (imax(QA, 1) - 1) / C - g_lo, QA - g_lo * C - C, QA - g_lo * C - 1, b, fullA);
        lin_band_range(lo_, 1, T_end, (imax(QB, 1) - 1) / C - g_lo, QB - g_lo * C - C, QB - g_lo * C - 1, b, fullB);
        lin_band_range(hi_, 0, T_end, (imax(QA, 1) - 1) / C - g_hi, QA - g_hi * C - C, QA - g_hi * C - 1, b, fullA);
        lin_band_range(hi_, 1, T_end, (imax(QB, 1) - 1) / C - g_hi, QB - g_hi * C - C, QB - g_hi * C - 1, b, fullB);
        bd = lo_;
        // (the quantum's highest lane may lie right of the tile -- dj_max < 0, nothing of its own to store: its hi is then the
        //  last step)
        bd.hi[0] = hi_.hi[0] < 0 ? (lo_.hi[0] < 0 ? lo_.hi[0] : T_end) : hi_.hi[0];
        bd.hi[1] = hi_.hi[1] < 0 ? (lo_.hi[1] < 0 ? lo_.hi[1] : T_end) : hi_.hi[1];
    }
    static_assert(!AMAX || LANES == kGroup, "first tiles run on the 16-lane layout");
    const int g = (int)(int16_t)(kc.ext & 0xffffu);
    const uint32_t gv = vconst(kc.next), g4v = vconst(kc.next4), c3v = vconst(kc.c3), onev = vconst(kc.one),
                   dtv = vconst(kc.next4 + kc.tag1),       // 4|g| + 1: G'' (tagged 2) -> D'' tagged 1
                   c2v = vconst(kc.tag2), lut1v = vconst(0x01010101u);
    uint32_t Z = pk2(lin_base(g) + gl * g);      // zero level of the row this lane did "before step 1"
    uint32_t G[C];                               // H of the previous row (see dp_pass_lin_split)
    uint32_t acc[2 * NW];
#pragma unroll
    for (int c = 0; c < C; c++) G[c] = Z;
#pragma unroll
    for (int c = 0; c < 2 * NW; c++) acc[c] = 0;
    uint32_t G_last = Z, Hdiag = Z;

    // arg-max state (see dp_pass_p16)
    uint32_t bk[AMAX ? C : 1];
    int lane_best[2] = {-1, -1};
    uint32_t col_x0 = 0;
    int t_first = 0, rows[2] = {0, 0};
    if (AMAX) {
#pragma unroll
        for (int c = 0; c < C; c++) bk[c] = 0xffffffffu;
        const int ncA = imin(imax(RQ[0][1] - gl * C, 0), C), ncB = imin(imax(RQ[1][1] - gl * C, 0), C);
        col_x0 = ((uint32_t)(-ncA) & 0xffffu) | ((uint32_t)(-ncB) << 16);
        t_first = gl + 1;
        rows[0] = RQ[0][0]; rows[1] = RQ[1][0];
    }

    auto lut = [&](uint32_t amount) { return kc.dsub >> (amount & 31u); };
    auto lut4 = [&](uint32_t amount) { return kc.dsub4 >> (amount & 31u); };
    uint32_t lutA = 0, lutB = 0;
    { const uint32_t w = ref16[1]; lutA = lut(w & 0xffu); lutB = lut(w >> 8); }

    auto shr1 = [](uint32_t v, uint32_t old) {
        return (uint32_t)(LANES == 32 ? dpp_shr1_32((int)v, (int)old) : dpp_row_shr1((int)v, (int)old));
    };

    // (stages of one instruction kind over all slots, as in dp_pass_lin_split)
#define GACT_SB() __builtin_amdgcn_sched_barrier(0)
    auto upper_all = [&](uint32_t (&U)[C], const bool tag2, const uint32_t Zr) {
        uint32_t P[C];
#pragma unroll
        for (int c = 0; c < C; c++) P[c] = __builtin_amdgcn_perm(lutB, lutA, qb[c]);
        GACT_SB();
#pragma unroll
        for (int c = 0; c < C; c++) U[c] = (c == 0 ? Hdiag : G[c - 1]) + P[c];                 // align.cpp:134-144
        (void)tag2;                              // (pointer phase: G is kept tagged 2 = H_up'' as it stands, see dp_pass_lin_split)
        GACT_SB();
        if (GACT_LIN_MAX3) {
#pragma unroll
            for (int c = 0; c < C; c++) U[c] = pk_max3f(U[c], Zr, G[c]);                       // :145-147 and the insertion, :149-154
        } else {
#pragma unroll
            for (int c = 0; c < C; c++) U[c] = lin_max(U[c], Zr);                               // :145-147
            GACT_SB();
#pragma unroll
            for (int c = 0; c < C; c++) U[c] = lin_max(U[c], G[c]);                             // the insertion, :149-154
        }
        GACT_SB();
    };

    auto step = [&](const int t) {
        const uint32_t w_next = ref16[t + 1];
        Z += gv;
        const uint32_t Hl0 = shr1(G_last, Z);            // j = 0 border: the zero level
        uint32_t U[C];
        upper_all(U, false, Z);
        Hdiag = Hl0;
        uint32_t Hl = Hl0;
#pragma unroll
        for (int c = 0; c < C; c++) { G[c] = lin_max(U[c], Hl - gv); Hl = G[c]; }               // :151-160
        G_last = Hl;
        lutA = lut(w_next & 0xffu); lutB = lut(w_next >> 8);
    };

    uint32_t Z4 = 0, Z8 = 0;
    auto step_tagged = [&](const int t) {
        const uint32_t w_next = ref16[t + 1];
        Z4 += g4v;
        uint32_t key_c = 0;
        if (AMAX) {
            Z8 += g4v + g4v;
            const uint32_t sidx = (uint32_t)(t - tB) & 7u, row0 = (uint32_t)(t - t_first);
            const uint32_t ka = row0 < (uint32_t)rows[0] ? sidx : ((uint32_t)kKeyBias & 0xffffu);
            const uint32_t kb = row0 < (uint32_t)rows[1] ? sidx : ((uint32_t)kKeyBias & 0xffffu);
            key_c = lin_sub(ka | (kb << 16), Z8);
        }
        const uint32_t Hl0 = shr1(G_last, Z4 - onev);       // j = 0 border: the zero level, tagged 2 like every G''
        uint32_t U[C];
        upper_all(U, true, Z4);
        Hdiag = Hl0;
        uint32_t Hl = Hl0, tprev = 0;
#pragma unroll
        for (int c = 0; c < C; c++) {
            const uint32_t Db = Hl - dtv;                                                       // G'' tagged 2 -> D'' tagged 1
            GACT_SB();
            const uint32_t Hp = lin_max(U[c], Db);                                               // the low bits: the op (:162-164)
            if (c > 0) {
                acc[c - 1] = pk_shl_add4(acc[c - 1], tprev);
                if (AMAX) bk[c - 1] = lin_max(bk[c - 1], pk_mad_vvv(G[c - 1], kc.tag2, key_c)); // 2 G'' + (step & 7) - Z8
            }
            GACT_SB();
            G[c] = andn_or(Hp, c3v, c2v);                                                       // low bits := 2
            tprev = Hp & c3v;
            GACT_SB();
            Hl = G[c];
        }
        acc[C - 1] = pk_shl_add4(acc[C - 1], tprev);
        if (AMAX) bk[C - 1] = lin_max(bk[C - 1], pk_mad_vvv(G[C - 1], kc.tag2, key_c));
        G_last = Hl;
        lutA = lut4(w_next & 0xffu) + lut1v; lutB = lut4(w_next >> 8) + lut1v;
    };
#undef GACT_SB
    auto enter_tagged = [&]() {
#pragma unroll
        for (int c = 0; c < C; c++) G[c] = pk_mad4v(G[c], c2v);
        G_last = pk_mad4v(G_last, c2v);
        Hdiag = pk_mad4v(Hdiag, c2v);
        Z4 = pk_mad4v(Z, c3v);                          // the zero level itself stays tagged 3
        Z8 = Z4 + Z4 - c2v;                             // 8 Z + 4 = twice a zero-score G'': the keys are 8 (H - Z) + (step & 7)
        lutA = (lutA << 2) + lut1v; lutB = (lutB << 2) + lut1v;
    };

    // fold the block keys of stored steps kblk..kblk+7 into lane_best (as dp_pass_p16)
    auto fold = [&](const int kblk) {
        uint32_t m = 0xffffffffu, rel = 0, x = col_x0;
#pragma unroll
        for (int c = 0; c < C; c++) {
            const uint32_t v = pk_sign(x);
            x = pk_add(x, kc.one);
            const uint32_t key = pk_mad_m1(v, pk_add(bk[AMAX ? c : 0], kc.one));
            const uint32_t keep = pk_sign(lin_sub(key, m));
            rel = pk_mad_m1(keep, rel);
            m = lin_max(m, key);
            bk[AMAX ? c : 0] = 0xffffffffu;
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int m16 = (int)(m << (16 - 16 * h)) >> 16;
            const int col = ((int)(rel << (16 - 16 * h)) >> 16) + C;
            const int rec = ((m16 >> 3) << 15) | ((kblk + (m16 & 7)) << 5) | col;
            lane_best[h] = imax(lane_best[h], m16 < 0 ? -1 : rec);
        }
    };

    int t = 1;
    for (; t < tB && t <= T_end; t++) step(t);
    const bool tagged = t <= T_end;
    if (tagged) enter_tagged();
    uint4 *qA = reinterpret_cast<uint4 *>(wsA) + gl;
    uint4 *qB = reinterpret_cast<uint4 *>(wsB) + gl;
    int k = 0;
    while (t + 7 <= T_end) {                     // whole blocks of eight steps + flush (see dp_pass_lin_split)
        for (int s8 = 0; s8 < 8; s8++, t++) step_tagged(t);
        k += 8;
        lin_flush<NW, LANES>(acc, qA, qB, [](uint32_t w) { return w; }, store && bd.store(0, t - 8, t - 1), store && bd.store(1, t - 8, t - 1));
        qA += QD * kWsRow;
        qB += QD * kWsRow;
        if (AMAX) fold(k - 8);
    }
    for (; t <= T_end; t++, k++) step_tagged(t);
    if (AMAX) {
        if (k & 7) fold(k & ~7);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int rec = lane_best[h];
            int best = 0, bi = 0, bj = 0;                               // align.cpp:109-112
            if (rec >= 0) {
                best = rec >> 15;
                bi = tB + ((rec >> 5) & 1023) - gl;
                bj = gl * C + (rec & 31) + 1;
            }
#pragma unroll
            for (int mm = 1; mm < kGroup; mm <<= 1) {
                const int ob = __shfl_xor(best, mm, kGroup);
                const int oi = __shfl_xor(bi, mm, kGroup);
                const int oj = __shfl_xor(bj, mm, kGroup);
                const bool take = (ob > best) | ((ob == best) & ((oi > bi) | ((oi == bi) & (oj > bj))));
                best = take ? ob : best;
                bi = take ? oi : bi;
                bj = take ? oj : bj;
            }
            pb->best[h] = best; pb->bi[h] = bi; pb->bj[h] = bj;
        }
    }
    if (k & 7) {
        const int sh = 2 * (8 - (k & 7));
        lin_flush<NW, LANES>(acc, qA, qB, [sh](uint32_t w) { return ((w & 0xffffu) << sh & 0xffffu) | ((w >> 16) << sh << 16); },
                             store && bd.store(0, t - (k & 7), t - 1), store && bd.store(1, t - (k & 7), t - 1));
    }
    if (AMAX) return 0;
    // H[R][Q]: slot cq of the lane that owns column Q, at the row of the last step; drift taken off
    uint32_t ga = G[0], gb = G[0];
#pragma unroll
    for (int c = 1; c < C; c++) { ga = (c == cqA) ? G[c] : ga; gb = (c == cqB) ? G[c] : gb; }
    const uint32_t pick = __builtin_amdgcn_perm(gb, ga, 0x07060100u);           // {tile B's half of gb, tile A's half of ga}
    return tagged ? pk_ashr2(lin_sub(pick | kc.c3, Z4)) : lin_sub(pick, Z);
}

// The wide main launch of linear scorings: UniformLayout<10, 32>'s column map, the pass above, FMT 3 words
struct WideLayoutLin : UniformLayout<10, 32, true> {
    static constexpr int kWalkFmt = 3, kWalkQuads = LinWords<10>::kUint4;
#ifndef GACT_WALK_SPAN
#define GACT_WALK_SPAN 16
#endif
    static constexpr int kWalkSpan = GACT_WALK_SPAN;          // region cache of the look-ahead walker (gact_chain.hpp)
#ifndef GACT_WIDE_LIN_BLOCKS
#define GACT_WIDE_LIN_BLOCKS 3
#endif
    static constexpr int kBlocksPerCu = GACT_WIDE_LIN_BLOCKS;  // launch bounds: waves per SIMD the register budget is cut for
    static constexpr bool kEndAligned = true;
    template <bool RAW>
    __device__ static uint32_t pass(const P16Consts &kc, int gl, const uint16_t *ref16, const uint32_t (&qb)[10], int T_end,
                                    int tB, uint32_t *wsA, uint32_t *wsB, const PairTile &pt)
    {
        static_assert(!RAW, "the linear-gap pass reads 2-bit sets");
        return dp_pass_lin<10, 32, false>(kc, gl, ref16, qb, T_end, tB, wsA, wsB, (imax(pt.Q[0], 1) - 1) % 10,
                                          (imax(pt.Q[1], 1) - 1) % 10, nullptr, nullptr, pt.col_from, pt.band, pt.Q[0], pt.Q[1],
                                          pt.full[0], pt.full[1]);
    }
    __device__ static int fin_lane(int Q) { return (imax(Q, 1) - 1) / 10; }
};

// Layout policy for extend_p16_kernel: SplitLayout's column map, the linear-gap pass, FMT 3 pointer words
#ifndef GACT_LIN_BLOCKS_PER_CU
#define GACT_LIN_BLOCKS_PER_CU 3
#endif
template <int C1, int C2> struct SplitLayoutLin : SplitLayout<C1, C2, true> {
    static constexpr int kBlocksPerCu = GACT_LIN_BLOCKS_PER_CU;
    static constexpr int kWalkFmt = 3, kWalkQuads = LinWords<C2>::kUint4;
    static constexpr int kWalkSpan = GACT_WALK_SPAN;
    static constexpr bool kEndAligned = true;       // every tile's last row on the wave's last step
    static constexpr int kLutWords = kLinLutWords;  // the kernel keeps the pass's table and hands it over in PairTile::lut
    static constexpr bool kColDrift = true;         // the column-drifted pass and lin_lut_fill_col's words (2b., 12.)
    using Base = SplitLayout<C1, C2, true>;
    template <bool RAW>
    __device__ static void load(const SeqSetDev &rs, const SeqSetDev &qf, const SeqSetDev &qr,
                                const PairTile &pt, int gl, uint8_t *ref8, uint8_t *q8, uint32_t (&qb)[C1 + C2], uint32_t *stage)
    {
        static_assert(!RAW, "the linear-gap pass reads 2-bit sets");
        load_pair_packed<C1 + C2, kGroup, typename Base::Cols, true, kLinPadRow>(rs, qf, qr, pt, gl, ref8, Base::G::kRefBytes, Base::G::kRow0, q8,
                                                                                 Base::G::kTileMax, qb, stage, typename Base::Cols{});
    }
    template <bool RAW>
    __device__ static uint32_t pass(const P16Consts &kc, int gl, const uint16_t *ref16, const uint32_t (&qb)[C1 + C2],
                                    int T_end, int tB, uint32_t *wsA, uint32_t *wsB, const PairTile &pt)
    {
        static_assert(!RAW, "the linear-gap pass reads 2-bit sets");
        return dp_pass_lin_split_col<C1, C2>(kc, gl, ref16, qb, T_end, tB, wsA, wsB, pt.band, pt.full[0], pt.full[1], pt.lut);
    }
    // lane and half-word of pass()'s return value that hold H[R][Q] of slot h
    __device__ static int fin_lane(int Q) { (void)Q; return kGroup - 1; }
};

// The same launch on the row-drifted pass, for the linear scorings whose pointer byte does not fit the column-drifted frame
// (lin_col_drift_ok, 12. above).  A kernel symbol of its own: the names with SplitLayoutLin stay the column-drifted pass's.
template <int C1, int C2> struct SplitLayoutLinRow : SplitLayoutLin<C1, C2> {
    static constexpr bool kColDrift = false;
    template <bool RAW>
    __device__ static uint32_t pass(const P16Consts &kc, int gl, const uint16_t *ref16, const uint32_t (&qb)[C1 + C2],
                                    int T_end, int tB, uint32_t *wsA, uint32_t *wsB, const PairTile &pt)
    {
        static_assert(!RAW, "the linear-gap pass reads 2-bit sets");
        return dp_pass_lin_split<C1, C2>(kc, gl, ref16, qb, T_end, tB, wsA, wsB, pt.band, pt.full[0], pt.full[1], pt.lut);
    }
};

template <int C1, int C2> struct SplitLayoutLinRowTeam : SplitLayoutLinRow<C1, C2> {      // (with the look-ahead walker, as below)
    static constexpr bool kTeamWalk = true;
};

// The same launch with the look-ahead walker (teams of eight lanes, gact_chain.hpp).  Alone on the machine the team makes
// the split launch slower (+5 % on ecoli10x: a wave iteration lasts longer, and that is what a run waits for); with several
// runs in flight what counts is instructions and the team walks in a third of the loop trips: +1.6 % with the team in every
// launch, +0.3 % (noise) when only the launches that share the machine take it (round 4, profiles/r04/ab_team_walker.txt).
// Off by default; GACT_HIP_TEAM_WHEN_SHARED=1 makes the engine take this variant for a launch that shares the machine.
template <int C1, int C2> struct SplitLayoutLinTeam : SplitLayoutLin<C1, C2> {
    static constexpr bool kTeamWalk = true;
};

}  // namespace gact
