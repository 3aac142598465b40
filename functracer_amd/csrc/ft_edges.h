// ft_edges.h — the edge record of a projected triangle (option "edge_cull"): what k_block_lists writes beside every entry
// of a candidate list and k_ls_edges beside every entry of a shadow grid, and the wave-level test mesh_list_closest and mesh_shadow_grid
// make of it.  Device code only; tests/edge_tools.py is its numpy twin, operation for operation.
//
// A record is three lines (a, b, c) as floats, nine in all.  Every point (x, y) of the plane from which a ray can get a hit out of
// tri_hit_wave on the triangle satisfies a x + b y + c <= 0 for all three - also as the wave test evaluates it in float - or the record
// is the SENTINEL, nine zeros, which cuts nothing off.  The plane is the one the entry's rectangle lives in: (jx, jy) of the primaries,
// (u, v) of a pair's frame.
//   The line of an edge: its unit normal pointing away from the third vertex, rounded to float (af, bf); d = the largest af x + bf y
//   over the three vertices, in FP64 with the rounded normal, so the rounding of the normal moves the line but never past a vertex.
//   The margin m = (|af| + |bf|) E + 1e-6 (|af| X + |bf| Y + |d|), E the inflation the entry's rectangle already carries on each axis (the
//   rectangle says: a hit comes from within E of the triangle's bounding rectangle; the record says: from within the box of half-width E
//   around a point of the triangle), X and Y the largest |x| + E and |y| + E of the vertices.  The second term covers the wave test's
//   float arithmetic: min(af x0, af x1) + min(bf y0, bf y1) + c rounds three times, each by at most 6e-8 of a value no larger than
//   |af| X + |bf| Y + |c| at a point the inflated triangle holds, and a float product and a float sum are monotone, so the value at the
//   wave's rectangle is no larger than the value at any of its points.  c = -(d + m), rounded down.
//   Sentinel where the rectangle is unbounded; where twice the area is not above 2e-6 of the longest edge squared (area / edge^2 <= 1e-6: a
//   sliver, or a triangle seen edge on - the barycentrics of tri_hit_wave lose their digits there, and only the rectangle argument holds);
//   where m is not below 5e-3 of the rectangle's width + height (a triangle so small against its coordinates that the float slack is no
//   longer small against it: the lines would cut nothing the rectangle does not); where anything is not finite.  Every test is written so
//   that a NaN fails it towards the sentinel.
#ifndef FT_EDGES_H
#define FT_EDGES_H
#include <hip/hip_runtime.h>

#include "ft_device.h"

namespace ftk {

constexpr double kEdgeSliver = 2e-6, kEdgeFloatSlack = 1e-6, kEdgeMaxMargin = 5e-3;

// x, y: the projected vertices; E: the inflation of the entry's rectangle; bounded: that rectangle is finite.  rec: nine floats.
__device__ __forceinline__ void edge_record(const double (&x)[3], const double (&y)[3], double E, bool bounded, float (&rec)[kEdgeFloats]) {
    const double w = fmax(x[0], fmax(x[1], x[2])) - fmin(x[0], fmin(x[1], x[2])), h = fmax(y[0], fmax(y[1], y[2])) - fmin(y[0], fmin(y[1], y[2]));
    const double X = fmax(fabs(x[0]), fmax(fabs(x[1]), fabs(x[2]))) + E, Y = fmax(fabs(y[0]), fmax(fabs(y[1]), fabs(y[2]))) + E;
    const double area2 = fabs(__dsub_rn(__dmul_rn(x[1] - x[0], y[2] - y[0]), __dmul_rn(x[2] - x[0], y[1] - y[0])));
    double l2 = 0.0;
    bool ok = bounded && E >= 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        const double ex = x[j] - x[i], ey = y[j] - y[i];
        const double len2 = __dadd_rn(__dmul_rn(ex, ex), __dmul_rn(ey, ey));
        l2 = fmax(l2, len2);
        const double len = sqrt(len2);
        double a = ey / len, b = -ex / len;
        const double side = __dadd_rn(__dmul_rn(a, x[k] - x[i]), __dmul_rn(b, y[k] - y[i]));
        if (side > 0.0) { a = -a; b = -b; }
        const float af = (float)a, bf = (float)b;
        double d = -__builtin_inf();
#pragma unroll
        for (int v = 0; v < 3; ++v) d = fmax(d, __dadd_rn(__dmul_rn((double)af, x[v]), __dmul_rn((double)bf, y[v])));
        const double fa = fabs((double)af), fb = fabs((double)bf);
        const double m = __dadd_rn(__dmul_rn(fa + fb, E), __dmul_rn(kEdgeFloatSlack, __dadd_rn(__dadd_rn(__dmul_rn(fa, X), __dmul_rn(fb, Y)), fabs(d))));
        const double cd = -(d + m);
        const float cf = (float)(cd - __dadd_rn(__dmul_rn(2.4e-7, fabs(cd)), 1e-37));   // (round_down of k_block_lists)
        ok = ok && m < kEdgeMaxMargin * (w + h) && fabsf(af) + fabsf(bf) + fabsf(cf) < 3e38f;
        rec[3 * i] = af; rec[3 * i + 1] = bf; rec[3 * i + 2] = cf;
    }
    ok = ok && area2 > kEdgeSliver * l2;
    if (!ok) {
#pragma unroll
        for (uint32_t q = 0; q < kEdgeFloats; ++q) rec[q] = 0.0f;
    }
}

// The wave's rectangle [x0, x1] x [y0, y1] lies wholly outside one line of the record: no point of it can give a hit.  A sentinel, a NaN
// or an unbounded rectangle never says so.
__device__ __forceinline__ float edge_value(float a, float b, float c, float x0, float x1, float y0, float y1) {
    return fminf(a * x0, a * x1) + fminf(b * y0, b * y1) + c;
}
__device__ __forceinline__ bool edges_outside(const float* rec, float x0, float x1, float y0, float y1) {
    const float t0 = edge_value(rec[0], rec[1], rec[2], x0, x1, y0, y1), t1 = edge_value(rec[3], rec[4], rec[5], x0, x1, y0, y1), t2 = edge_value(rec[6], rec[7], rec[8], x0, x1, y0, y1);
    return t0 > 0.0f || t1 > 0.0f || t2 > 0.0f;
}

} // namespace ftk
#endif
