// lin_taps.h -- the float32 INTER_LINEAR tap rule shared by paste.hip and sampleprep.hip (oracle/paste.py states it: the published
// generic path of OpenCV's resize.cpp for CV_32F).  Include only from translation units compiled with -ffp-contract=off: every
// product and sum must round as written (horizontal pass first, float32).
#pragma once
#include <math.h>

struct Taps { int s0, s1; float c0, c1; int single; };
// destination index d of a resize ssize -> dsize; horizontal = OpenCV's xofs/alpha (border taps collapsed, single tap from xmax
// on), vertical = rows clamped with unchanged coefficients
__device__ __forceinline__ Taps lin_taps(int d, int ssize, int dsize, bool horizontal) {
    Taps t;
    const double scale = 1.0 / ((double)dsize / (double)ssize);
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (horizontal) {
        if (s < 0) { f = 0.f; s = 0; }
        if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
        t.single = s + 1 >= ssize;
        t.s0 = s; t.s1 = s + 1 < ssize ? s + 1 : ssize - 1;
    } else {
        t.single = 0;
        t.s0 = s < 0 ? 0 : (s > ssize - 1 ? ssize - 1 : s);
        t.s1 = s + 1 < 0 ? 0 : (s + 1 > ssize - 1 ? ssize - 1 : s + 1);
    }
    t.c0 = 1.f - f; t.c1 = f;
    return t;
}
__device__ __forceinline__ float lin_row(float v0, float v1, const Taps& t) {
    if (t.single) return v0;
    const float a = v0 * t.c0, b = v1 * t.c1;
    return a + b;
}
