// f110_noise.h -- the lidar noise of the step path, generated on the GPU.
//
// Reference: every scan of every car adds `rng.normal(0., 0.01, size=num_beams)` (laser_models.py:450-452) drawn from a
// per-car `np.random.default_rng(seed)` that is re-created at every reset (base_classes.py:117,202).  All cars of an env
// share the seed, so the row a car adds depends only on (seed, scans since its reset): the rows of one seed are kept
// ONCE per seed ("noise slot") in a device table indexed by each car's own counter, and produced here, on the device,
// by a bit-level restatement of what NumPy executes for that call:
//   * PCG64 (numpy/random/src/pcg64/pcg64.h, pcg_setseq_128_xsl_rr_64): 128-bit LCG step, XSL-RR output of the new state;
//   * random_standard_normal (numpy/random/src/distributions/distributions.c): 256-layer ziggurat -- 99.3 % of the draws
//     are one table compare; the wedge test uses exp(), the tail (|x| > 3.654, 0.026 % of the draws) log1p();
//   * random_normal: loc + scale * x.
// The stream is sequential (a draw consumes one raw value, or more after a rejection), so ONE WAVEFRONT per seed walks it,
// 64 raw values at a time (noise_rows_kernel in f110_noise_kernels.h; lane j holds the generator state of raw position p + j by LCG
// jump-ahead).  Exactness: every accepted value outside the tail is the product of an integer and a table entry (no library
// call); the wedge test compares against exp() (a decision, and the only one a library rounding could flip: none has been
// seen in 1e8 draws); the tail's log1p is glibc's own sequence of roundings (log1p_glibc below), so the rows are NumPy's bits.
#pragma once
#include "f110_device.h"
#include "f110_ziggurat.h"

#pragma clang fp contract(off)

namespace f110 {

typedef unsigned __int128 u128;

// What the scan kernel needs to find a car's noise row.  Lives in device memory at an address that never changes for
// the handle's life (the kernel's by-value arguments -- and therefore captured hipGraphs -- survive every growth).
// Row r of slot s: base[(s * cap + (r & mask)) * num_beams + beam] = the beam's noise; rows lo <= r < hi are present (a ring once
// lo > 0); noise off: cap = 1, one row of zeros.  (Rounds 3-4 kept {noise, side distance} pairs here so that one gather fed the
// iTTC test as well; once the cars of a batch stand on different rows the rows stream from L2 / HBM, and the 8 redundant bytes per
// beam cost 4.6 % of a 65 536-car launch -- the side distance is now read only for iTTC candidates, profiles/r04_scan_stores.txt M.)
struct NoiseDesc {
    const double *base;
    int mask, cap, lo, hi; // (a car's row counter is an int32: f110_buffers.noise_step)
    int slots, pad;        // slots the table holds (read by the bounds-checked build only)
};

// generator of one slot: t = the LCG state whose output is the NEXT raw value of the stream
struct NoiseGen {
    unsigned long long t_lo, t_hi, inc_lo, inc_hi;
    double std;
    long long rows;   // rows produced so far (the stream stands at the start of row `rows`)
    int on, pad;
};

__device__ inline u128 pcg_mult() { return ((u128)0x2360ED051FC65DA4ull << 64) | (u128)0x4385DF649FCCF645ull; } // PCG_DEFAULT_MULTIPLIER_128

__device__ inline unsigned long long pcg_out(u128 s) // pcg_output_xsl_rr_128_64
{
    const unsigned long long hi = (unsigned long long)(s >> 64), lo = (unsigned long long)s;
    const unsigned long long x = hi ^ lo;
    const unsigned rot = (unsigned)(hi >> 58);
    return (x >> rot) | (x << ((0u - rot) & 63u));
}

__device__ inline double pcg_double(unsigned long long raw) { return (double)(raw >> 11) * (1.0 / 9007199254740992.0); }

__device__ inline u128 shfl128(u128 v, int src)
{
    unsigned w0 = (unsigned)v, w1 = (unsigned)(v >> 32), w2 = (unsigned)(v >> 64), w3 = (unsigned)(v >> 96);
    w0 = (unsigned)__shfl((int)w0, src); w1 = (unsigned)__shfl((int)w1, src);
    w2 = (unsigned)__shfl((int)w2, src); w3 = (unsigned)__shfl((int)w3, src);
    return ((u128)w3 << 96) | ((u128)w2 << 64) | ((u128)w1 << 32) | (u128)w0;
}

__device__ inline unsigned long long shfl64(unsigned long long v, int src)
{
    const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

// the stream of a slot at the start of row 64 * k (its LCG state): written when the row is first reached, so that rows which
// were dropped from the ring can be produced again from the nearest mark -- in parallel, one wavefront per 64 rows -- instead of
// from the seed
struct NoiseMark { unsigned long long t_lo, t_hi; };
constexpr int NOISE_MARK_ROWS = 64;

// log1p as glibc computes it (sysdeps/ieee754/dbl-64/s_log1p.c, 2.35: the fdlibm algorithm -- argument reduction to
// 1 + f in [sqrt(2)/2, sqrt(2)), the degree-7 polynomial in z = (f / (2 + f))^2 regrouped as R1 + z2*R2 + z4*R3 + z6*R4 --
// built for x86-64 without contraction), restated operation by operation: NumPy's ziggurat calls the C library's log1p for
// its tail draws (0.026 % of the draws), and fdlibm's result is within an ulp of the true value but not the correctly rounded
// one, so "NumPy's bits" means this sequence of roundings.  tools/log1p_model.py is the same text in Python, compared with
// the local libm bit for bit over 5e5 arguments (and the libm's constants read from its binary); the device math library's
// log1p differed in 4 of 2 156 tail draws (round 4).  Domain here: x = -u, u in [0, 1).
__device__ inline double log1p_glibc(double x)
{
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    const double Lp1 = 6.666666666666735130e-01, Lp2 = 3.999999999940941908e-01, Lp3 = 2.857142874366239149e-01,
                 Lp4 = 2.222219843214978396e-01, Lp5 = 1.818357216161805012e-01, Lp6 = 1.531383769920937332e-01,
                 Lp7 = 1.479819860511658591e-01;
    const int hx = __double2hiint(x);
    const int ax = hx & 0x7fffffff;
    int k = 1, hu = 1;
    double f = 0.0, c = 0.0;
    if (hx < 0x3FDA827A) {                                  // x < 0.41422
        if (ax >= 0x3ff00000) return x == -1.0 ? -__builtin_inf() : __builtin_nan(""); // x <= -1 (not reached: u < 1)
        if (ax < 0x3e200000) {                              // |x| < 2^-29
            if (ax < 0x3c900000) return x;                  // |x| < 2^-54
            return x - x * x * 0.5;
        }
        if (hx > 0 || hx <= (int)0xbfd2bec3) { k = 0; f = x; hu = 1; } // -0.2929 < x < 0.41422
    } else if (hx >= 0x7ff00000) return x + x;
    if (k != 0) {
        double u;
        if (hx < 0x43400000) {
            u = 1.0 + x;
            hu = __double2hiint(u);
            k = (hu >> 20) - 1023;
            c = (k > 0) ? 1.0 - (u - x) : x - (u - 1.0);    // correction term
            c = c / u;
        } else {
            u = x;
            hu = __double2hiint(u);
            k = (hu >> 20) - 1023;
            c = 0.0;
        }
        hu &= 0x000fffff;
        if (hu < 0x6a09e) u = __hiloint2double(hu | 0x3ff00000, __double2loint(u));           // normalize u
        else { k += 1; u = __hiloint2double(hu | 0x3fe00000, __double2loint(u)); hu = (0x00100000 - hu) >> 2; } // normalize u / 2
        f = u - 1.0;
    }
    const double hfsq = (0.5 * f) * f;
    if (hu == 0) {                                          // |f| < 2^-20
        if (f == 0.0) {
            if (k == 0) return 0.0;
            c = c + (double)k * ln2_lo;
            return (double)k * ln2_hi + c;
        }
        const double R = hfsq * (1.0 - 0.66666666666666666 * f);
        if (k == 0) return f - R;
        return (double)k * ln2_hi - ((R - ((double)k * ln2_lo + c)) - f);
    }
    const double s = f / (2.0 + f);
    const double z = s * s;
    const double R1 = z * Lp1, z2 = z * z;
    const double R2 = Lp2 + z * Lp3, z4 = z2 * z2;
    const double R3 = Lp4 + z * Lp5, z6 = z4 * z2;
    const double R4 = Lp6 + z * Lp7;
    const double R = ((R1 + z2 * R2) + z4 * R3) + z6 * R4;
    if (k == 0) return f - (hfsq - s * (hfsq + R));
    return (double)k * ln2_hi - ((hfsq - (s * (hfsq + R) + ((double)k * ln2_lo + c))) - f);
}

} // namespace f110
