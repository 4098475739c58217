"""CPU suite: the zero levels of the column-drifted split linear-gap pass (csrc/gact_lin.hpp 2b. and 13.) as the pass presents
them, step by step and slot by slot.

The pass keeps its zero levels in scalar registers.  Inside a whole block of eight steps they form a strip that covers the
block, step S reading strip[S + k]; the strip moves once per block; the steps outside whole blocks move a window of levels
by one gap per step.  The bookkeeping -- which entry a step reads (lin_strip_at), the move behind a block (lin_strip_slide),
the hand-over between the two forms (lin_strip_enter, lin_strip_leave) -- is host-callable, and the program below drives
exactly those helpers through the loop structure of dp_pass_lin_split_col<7, 13>: the steps of region 1 alone, the plain
steps (whole trips of eight and the steps left over), the pointer phase's blocks of both regions and of region 2 alone, and
the remainder.  Checked at every step and slot: the level presented is lin_base + (t + c)|g| in both half-words (the j = 0
border: c = -1), scaled 4 * ... + 3 for region 2 in the pointer phase, and so is the level the pass's return value takes off.

Passes: a non-first tile (early = 200) and a first-tile-like one (early = the tile) of every size 1..320 with R = Q; R != Q
over the sizes of tests/test_gpu_lin_level_window.py; and, at sizes on either side of every change of the block structure,
every step at which the pointer phase can begin, 1 .. T_end + 1 (none).  g in {0, -1, -12}.  The program is built with the
slide and with -DGACT_LIN_SLIDE=0 (the per-step additions)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstdio>
#include <cstdlib>
#include "gact_lin.hpp"
using namespace gact;
constexpr int C1 = 7, C2 = 13, LAG = kGroup, NWIN = C2 + 1;
static long long checks = 0, kinds[8];
static int imin(int a, int b) { return a < b ? a : b; }      // (host twins of gact_device.hpp's)
static int imax(int a, int b) { return a > b ? a : b; }
static int g, T_end, tB;
static uint32_t Zw(int k) { return pk2(lin_base(g) + k * (-g)); }
static void expect(uint32_t got, uint32_t want, const char *what, int t, int c)
{
    checks++;
    if (got != want) {
        printf("FAIL g %d T_end %d tB %d: %s step %d slot %d presents %08x, not %08x\n", g, T_end, tB, what, t, c, got, want);
        exit(1);
    }
}
static uint32_t scaled(uint32_t z) { return (z << 2) + 0x00030003u; }
// the loop structure of dp_pass_lin_split_col, levels only
static void pass()
{
    const uint32_t gs = pk2(-g), g4s = pk2(-4 * g);
    uint32_t W[lin_strip_len(NWIN)] = {}, T[lin_strip_len(C2)] = {};
    for (int k = 0; k < NWIN; k++) W[k] = pk2(lin_base(g) + (k - 1) * (-g));
    auto add1 = [](uint32_t &z, uint32_t by) { z += by; };
    auto add4 = [](uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d, uint32_t by) { a += by; b += by; c += by; d += by; };
    auto advance = [&](int nW, bool tagged_too) {
        for (int k = 0; k < nW; k++) W[k] += gs;
        if (tagged_too) for (int c = 0; c < C2; c++) T[c] += g4s;
    };
    int t = 1;
    auto step_r1 = [&]() {
        advance(C1 + 1, false);
        expect(W[0], Zw(t - 1), "step_r1 border", t, -1);
        for (int c = 0; c < C1; c++) expect(W[c + 1], Zw(t + c), "step_r1", t, c);
        kinds[0]++;
    };
    auto step = [&](int S) {
        const int o = lin_strip_at(S, 0);
        if (!GACT_LIN_SLIDE || S == kLinTail) advance(NWIN, false);
        expect(W[o], Zw(t - 1), "step border", t, -1);
        for (int c = 0; c < C1; c++) expect(W[lin_strip_at(S, c + 1)], Zw(t + c), "step region 1", t, c);
        for (int c = 0; c < C2; c++) expect(W[lin_strip_at(S, c + 1)], Zw(t + c), "step region 2", t, c);
        kinds[S == kLinTail ? 2 : 1]++;
    };
    auto step_tagged = [&](int S) {
        const int o = lin_strip_at(S, 0);
        if (!GACT_LIN_SLIDE || S == kLinTail) advance(C1 + 1, true);
        expect(W[o], Zw(t - 1), "step_tagged border", t, -1);
        for (int c = 0; c < C1; c++) expect(W[lin_strip_at(S, c + 1)], Zw(t + c), "step_tagged region 1", t, c);
        for (int c = 0; c < C2; c++) expect(T[lin_strip_at(S, c)], scaled(Zw(t + c)), "step_tagged region 2", t, c);
        kinds[S == kLinTail ? 4 : 3]++;
    };
    auto step_tagged_r2 = [&](int S) {
        if (!GACT_LIN_SLIDE || S == kLinTail) advance(0, true);
        for (int c = 0; c < C2; c++) expect(T[lin_strip_at(S, c)], scaled(Zw(t + c)), "step_tagged_r2", t, c);
        kinds[S == kLinTail ? 6 : 5]++;
    };
    for (const int tP = imin(LAG, imin(tB - 1, T_end)); t <= tP; t++) step_r1();
    if (t > 1) {
        for (int k = C1 + 1; k < NWIN; k++) W[k] = W[k - 1] + gs;
        // region 2 starts at its zero level, in the frame of step t - 1: what G[], H2, Hdiag2 take
        for (int c = 0; c < C2; c++) expect(W[c + 1], Zw(t - 1 + c), "region 2's start", t - 1, c);
        expect(W[0], Zw(t - 2), "region 2's start, diagonal", t - 1, -1);
    }
    const int tU = imin(tB - 1, T_end);
    if (GACT_LIN_SLIDE) {
        lin_strip_enter<NWIN>(W, gs);
        for (; t + kLinBlock - 1 <= tU; ) {
            for (int S = 0; S < kLinBlock; S++, t++) step(S);
            lin_strip_slide<NWIN>(W, gs * kLinBlock, add4, add1);
        }
        lin_strip_leave<NWIN>(W, gs);
    }
    for (; t + 1 <= tU; ) { step(kLinTail); t++; step(kLinTail); t++; }
    if (t <= tU) { step(kLinTail); t++; }
    const bool tagged = t <= T_end;
    if (tagged) for (int c = 0; c < C2; c++) T[c] = scaled(W[c + 1]);           // enter_tagged
    if (GACT_LIN_SLIDE && tagged) { lin_strip_enter<C1 + 1>(W, gs); lin_strip_enter<C2>(T, g4s); }
    while (t + 7 <= T_end && t <= T_end - LAG) {
        for (int S = 0; S < 8; S++, t++) step_tagged(S);
        if (GACT_LIN_SLIDE) {
            lin_strip_slide<C1 + 1>(W, gs * kLinBlock, add4, add1);
            lin_strip_slide<C2>(T, g4s * kLinBlock, add4, add1);
        }
    }
    while (t + 7 <= T_end) {
        for (int S = 0; S < 8; S++, t++) step_tagged_r2(S);
        if (GACT_LIN_SLIDE) lin_strip_slide<C2>(T, g4s * kLinBlock, add4, add1);
    }
    if (GACT_LIN_SLIDE && tagged) { lin_strip_leave<C1 + 1>(W, gs); lin_strip_leave<C2>(T, g4s); }
    for (; t <= T_end - LAG; t++) step_tagged(kLinTail);
    for (; t <= T_end; t++) step_tagged_r2(kLinTail);
    // the drift the return value takes off: the last slot's level at the last step
    if (T_end >= 1) {
        if (tagged) expect(T[C2 - 1], scaled(Zw(T_end + C2 - 1)), "return value (pointer phase)", T_end, C2 - 1);
        else expect(W[C2], Zw(T_end + C2 - 1), "return value (plain)", T_end, C2 - 1);
    }
}
static int last_step(int R, int Q) { return (R > 0 && Q > 0) ? R + (kGroup - 1) + kGroup : 0; }        // split_last_step
static int first_pointer_step(int R, int Q, int early)                                                  // split_first_pointer_step
{
    const int r_first = imax(1, R - early + 1), j_first = imax(1, Q - early + 1);
    return r_first + (j_first + (C2 * kGroup - Q) - 1) / C2 + kGroup;
}
int main()
{
    const int gaps[3] = {0, -1, -12};
    static const int spans[4][2] = {{17, 64}, {120, 136}, {217, 232}, {289, 304}};
    static const int sweeps[] = {1, 2, 7, 8, 9, 15, 16, 17, 24, 25, 33, 64, 119, 120, 121, 136, 200, 201, 217, 304, 319, 320};
    long long passes = 0;
    for (int gi = 0; gi < 3; gi++) {
        g = gaps[gi];
        for (int x = 1; x <= 320; x++)
            for (int early : {200, x}) { T_end = last_step(x, x); tB = first_pointer_step(x, x, early); pass(); passes++; }
        for (auto &a : spans) for (auto &b : spans)
            for (int R = a[0]; R <= a[1]; R++) for (int Q = b[0]; Q <= b[1]; Q++) {
                if (R == Q) continue;
                T_end = last_step(R, Q); tB = first_pointer_step(R, Q, 200); pass(); passes++;
            }
        for (int x : sweeps) { T_end = last_step(x, x); for (tB = 1; tB <= T_end + 1; tB++) { pass(); passes++; } }
    }
    printf("ok slide %d passes %lld checks %lld kinds", GACT_LIN_SLIDE, passes, checks);
    for (int k = 0; k < 7; k++) printf(" %lld", kinds[k]);
    printf("\n");
    return 0;
}
'''


@pytest.fixture(scope="module")
def source(tmp_path_factory):
    d = tmp_path_factory.mktemp("lin_levels")
    (d / "t.hip").write_text(SRC)
    return d


@pytest.mark.parametrize("slide", (1, 0))
def test_levels_presented_at_every_step_and_slot(source, slide):
    exe = str(source / ("t%d" % slide))
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-DGACT_LIN_SLIDE=%d" % slide,
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "darwin-gpu_amd", "csrc"),
                           "-o", exe, str(source / "t.hip")])
    r = subprocess.run([exe], text=True, capture_output=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    words = r.stdout.split()
    assert words[:3] == ["ok", "slide", str(slide)], r.stdout
    kinds = [int(w) for w in words[words.index("kinds") + 1:]]
    # every kind of step was taken: region 1 alone, plain steps in whole trips (the slide only) and left over, pointer-phase
    # blocks of both regions, blocks of region 2 alone and their remainder.  (A remainder step of both regions does not
    # exist: region 1 stops LAG = 16 steps before the end, so a whole block always fits behind a step that still has it.)
    assert all(n > 0 for k, n in enumerate(kinds) if k != 4 and (slide or k != 1)), kinds
    assert kinds[4] == 0 and (slide or kinds[1] == 0), kinds
