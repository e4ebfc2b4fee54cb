// The vertex rule of a profile over a grid (step 4 of the ambient model in include/cellector_ffi.h), stated once for the passes that
// profile a scalar per cell: the ambient fraction rho (kernels_ambient.hip, and its host folds) and the share f of a donor pair
// (kernels_pair_fraction.hip).  One function: the two passes cannot drift apart by an operation.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#define AM_FLAT 0x1p-40  // two steps of a profile that both stay within this share of its value are rounding, not signal (the header)

// The vertex of the parabola through (x0, y0), (x1, y1), (x2, y2), the operations in the header's order.  curv = its second
// derivative, 0 where neither step of y is resolved (|y1 - y0| and |y2 - y1| both <= AM_FLAT |y1|).  curv < 0: est = the vertex
// clamped into [x0, x2], se = 1 / sqrt(-curv); otherwise (flat, convex, or not a number) est = flat, se = +inf.
__host__ __device__ static inline void am_vertex(double x0, double x1, double x2, double y0, double y1, double y2, double flat, double *est,
                                                 double *se, double *curv)
{
    const double h0 = x1 - x0, h1 = x2 - x1;
    const double e0 = y1 - y0, e1 = y2 - y1;
    const double d0 = e0 / h0, d1 = e1 / h1;
    const double dd = d1 - d0, hs = h0 + h1;
    const double two = 2.0 * dd;
    const double lim = AM_FLAT * fabs(y1);
    const bool resolved = fabs(e0) > lim || fabs(e1) > lim;
    const double c = resolved ? two / hs : 0.0;
    *curv = c;
    if (c < 0.0) {
        const double sx = x0 + x1;
        const double mid = 0.5 * sx;
        const double q = d0 / c;
        double v = mid - q;
        if (v < x0) v = x0;
        if (v > x2) v = x2;
        const double nc = -c;
        const double r = sqrt(nc);
        *est = v;
        *se = 1.0 / r;
    } else {
        *est = flat;
        *se = INFINITY;
    }
}
