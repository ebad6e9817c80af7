// The reference's training-free positional encoders 'Theory' (positional_encoding/theory.py:55-90) and
// 's2vec_*' (sphere2vec/sphere2vec.py:95-248: grid, spherec, spherecplus, spherem, spheremplus) - numpy on
// the host there - as one kernel, instantiated per kind.  Rows of 192 .. 512 float64, every entry a
// float64 sine or cosine (or a product of two) of a coordinate times a frequency; the coordinates are
// (lon, lat) DEGREES used as radians, as the reference does, so arguments reach 18 000 rad.
//
// WORK SPLIT.  One work item per (location, frequency): it evaluates sin/cos of its angles ONCE (two
// sincos for the s2vec kinds, three for Theory; the ocml float64 pair costs hundreds of instructions at
// these arguments) and emits all P = posenc_per_freq(kind) outputs of that frequency from registers.  The
// un-scaled sin(lon), cos(lon), cos(lat) of spherem / spheremplus are evaluated once per LOCATION by the
// first lanes of the workgroup and shared through LDS.  Items are numbered k = location * F + frequency; a
// workgroup takes tiles of 256 consecutive items and walks the tiles grid-stride (host_plan.h:
// posenc_plan; every index is 64-bit, B is unbounded).  No atomics, nothing waits on another workgroup.
//
// STORES.  For every kind but grid the P outputs of item k are the doubles [k P, (k + 1) P) of the output:
// a tile writes ONE contiguous run of 256 P doubles.  The lanes put their outputs into LDS and the
// workgroup writes the run out linearly, 16 bytes per lane, lanes contiguous - whole 128-byte lines per
// wave instruction.  (Measured against every lane storing its own run as P/2 16-byte stores, lanes P*8
// bytes apart: 0.62 - 0.96 of a device fill's rate staged, 0.52 - 0.62 direct; profiles/NOTES.md.)
// grid's row is two halves (lon | lat) of 2F doubles: a lane's two 16-byte stores are contiguous across
// the lanes of a location as they are, so grid stores from registers.  `out` must be 16-byte aligned
// (row widths are even).
//
// ROUNDING.  al = lon * f[i], at = lat * f[i]: one rounded multiply each.  Theory's angles a_j = lon * ux_j
// + lat * uy_j are two rounded multiplies and one rounded add (numpy's matmul of a (B,2) by a 2-vector):
// contracted into an FMA the angle's last bit changes (3e-14 in the output), so they are formed with
// contraction off.  lat * 0 is kept: a non-finite latitude makes a_1 NaN in the reference as well.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_plan.h"

namespace range_hip {

using range_host::POSENC_BLOCK;
using range_host::posenc_per_freq;
using range_host::PE_THEORY;
using range_host::PE_GRID;
using range_host::PE_SPHEREC;
using range_host::PE_SPHERECPLUS;
using range_host::PE_SPHEREM;
using range_host::PE_SPHEREMPLUS;

// x * ux + y * uy as two rounded products and one rounded sum, whatever -ffp-contract says
__device__ __forceinline__ double posenc_dot2_unfused(double x, double ux, double y, double uy) {
#pragma clang fp contract(off)
    const double p = x * ux;
    const double q = y * uy;
    return p + q;
}

// The sines and cosines of ONE (location, frequency) - what this kernel and the CSP encoders' feature
// phase (csp_kernel.h) both evaluate.  Theory: (sin, cos) of the three angles, v[0..5].
__device__ __forceinline__ void posenc_theory_item(double x, double y, double f, double* v) {
    constexpr double S3H = 1.7320508075688772 / 2.0;   // math.sqrt(3) / 2.0
    const double a1 = posenc_dot2_unfused(x, 1.0, y, 0.0);
    const double a2 = posenc_dot2_unfused(x, -0.5, y, S3H);
    const double a3 = posenc_dot2_unfused(x, -0.5, y, -S3H);
    sincos(a1 * f, &v[0], &v[1]);
    sincos(a2 * f, &v[2], &v[3]);
    sincos(a3 * f, &v[4], &v[5]);
}

// grid and the sphere kinds: (sin, cos) of lon * f and of lat * f
__device__ __forceinline__ void posenc_lonlat_item(double x, double y, double f, double& sal, double& cal, double& sat,
                                                   double& cat) {
    sincos(x * f, &sal, &cal);
    sincos(y * f, &sat, &cat);
}

struct PosencArgs {
    const double* freq;     // (F) float64, device
    const double* lonlat;   // (B,2) float64, (lon,lat) degrees
    double* out;            // (B, F * P) float64, 16-byte aligned
    int64_t B;
    int64_t n_tiles;        // ceil(B * F / 256)
    int32_t F;
};

template <int KIND>
__global__ __launch_bounds__(POSENC_BLOCK) void posenc_features_kernel(PosencArgs a) {
    constexpr int P = posenc_per_freq(KIND);
    constexpr bool SINGLE = KIND == PE_SPHEREM || KIND == PE_SPHEREMPLUS;   // needs sin/cos of the un-scaled coordinates
    constexpr bool STAGED = KIND != PE_GRID;                                 // the tile's run goes through LDS
    extern __shared__ __attribute__((aligned(16))) double pe_lds[];
    double* const stage = pe_lds;                                            // STAGED: 256 * P doubles
    double* const single = pe_lds + (STAGED ? POSENC_BLOCK * P : 0);         // SINGLE: 3 per location of the tile
    const int t = threadIdx.x;
    const int F = a.F;
    const int64_t n_items = a.B * F;
    double2* const out2 = reinterpret_cast<double2*>(a.out);
    for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int64_t k0 = tile * POSENC_BLOCK;
        const int64_t b0 = k0 / F;                       // first location of the tile (block-uniform)
        const unsigned r0 = (unsigned)(k0 - b0 * F);
        if constexpr (SINGLE) {
            // the tile's locations are b0 .. b0 + (r0 + 255) / F: at most 256 (host_plan.h: locs_per_tile)
            const unsigned n_loc = (r0 + POSENC_BLOCK - 1) / (unsigned)F + 1;
            if ((unsigned)t < n_loc && b0 + t < a.B) {
                const double x = a.lonlat[2 * (b0 + t)], y = a.lonlat[2 * (b0 + t) + 1];
                double sx, cx;
                sincos(x, &sx, &cx);
                single[3 * t + 0] = sx;
                single[3 * t + 1] = cx;
                single[3 * t + 2] = cos(y);
            }
            __syncthreads();
        }
        const unsigned u = r0 + (unsigned)t;
        const unsigned db = u / (unsigned)F;             // location within the tile
        const int i = (int)(u - db * (unsigned)F);       // frequency
        const int64_t b = b0 + db;
        const bool live = k0 + t < n_items;
        double v[P];
        if (live) {
            const double x = a.lonlat[2 * b], y = a.lonlat[2 * b + 1];
            const double f = a.freq[i];
            if constexpr (KIND == PE_THEORY) {
                posenc_theory_item(x, y, f, v);
            } else {
                double sal, cal, sat, cat;
                posenc_lonlat_item(x, y, f, sal, cal, sat, cat);
                if constexpr (KIND == PE_GRID) {
                    v[0] = sal; v[1] = cal; v[2] = sat; v[3] = cat;
                } else if constexpr (KIND == PE_SPHEREC) {
                    v[0] = v[1] = sat;
                    v[2] = v[3] = cat * cal;
                    v[4] = v[5] = cat * sal;
                } else if constexpr (KIND == PE_SPHERECPLUS) {
                    v[0] = v[1] = sat;
                    v[2] = v[3] = cat;
                    v[4] = v[5] = sal;
                    v[6] = v[7] = cal;
                    v[8] = v[9] = cat * cal;
                    v[10] = v[11] = cat * sal;
                } else {
                    const double sx = single[3 * db + 0], cx = single[3 * db + 1], cy = single[3 * db + 2];
                    constexpr int o = KIND == PE_SPHEREMPLUS ? 6 : 0;
                    v[0] = v[1] = sat;
                    if constexpr (KIND == PE_SPHEREMPLUS) {
                        v[2] = v[3] = cat;
                        v[4] = v[5] = sal;
                        v[6] = v[7] = cal;
                    }
                    v[o + 2] = v[o + 3] = cat * cx;
                    v[o + 4] = v[o + 5] = cy * cal;
                    v[o + 6] = v[o + 7] = cat * sx;
                    v[o + 8] = v[o + 9] = cy * sal;
                }
            }
            if constexpr (KIND == PE_GRID) {
                // row b = [ lon half: 2F | lat half: 2F ]; (sin, cos) of frequency i at 2i of each half
                const int64_t row2 = b * (2 * F);        // in double2 units: the row is 4F doubles
                out2[row2 + i] = make_double2(v[0], v[1]);
                out2[row2 + F + i] = make_double2(v[2], v[3]);
            } else {
                double2* const s2 = reinterpret_cast<double2*>(stage) + t * (P / 2);
#pragma unroll
                for (int j = 0; j < P / 2; ++j) s2[j] = make_double2(v[2 * j], v[2 * j + 1]);
            }
        }
        if constexpr (STAGED) {
            __syncthreads();
            // the tile's run of 256 * P doubles, linearly: 16 bytes per lane, lanes contiguous
            const double2* const s2 = reinterpret_cast<const double2*>(stage);
            const int64_t g0 = k0 * (P / 2), g_end = n_items * (P / 2);
#pragma unroll
            for (int j = 0; j < P / 2; ++j) {
                const int idx = j * POSENC_BLOCK + t;
                if (g0 + idx < g_end) out2[g0 + idx] = s2[idx];
            }
        }
        if constexpr (STAGED || SINGLE) __syncthreads();   // the next tile overwrites the LDS
    }
}

}  // namespace range_hip

// Training-free coordinate encoders of the reference (range/range.py:262-272): one thread per
// location, float64.  mode 0 'Direct' (:262-264): (lon,lat)*pi/180, evaluated as (x*pi)/180 like
// the Python expression; mode 1 'Cartesian_3D' (:265-268, utils/utils.py:11-16): unit xyz of the
// radians above; mode 2 'Wrap' (positional_encoding/wrap.py:20-29): cos/sin of torch.deg2rad(x)
// = x * (pi/180) per column, ordered (cos lon, sin lon, cos lat, sin lat).
// (range_coord_features, encoder_host.h; extern "C": the symbol is the plain name)
extern "C" __global__ void coord_features_kernel(int mode, const double* __restrict__ lonlat, int64_t n,
                                      double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double lon = lonlat[2 * i], lat = lonlat[2 * i + 1];
    constexpr double PI = 3.141592653589793;
    if (mode == 2) {
        constexpr double PI_180 = 0.017453292519943295;
        const double a = lon * PI_180, b = lat * PI_180;
        out[4 * i + 0] = cos(a);
        out[4 * i + 1] = sin(a);
        out[4 * i + 2] = cos(b);
        out[4 * i + 3] = sin(b);
        return;
    }
    const double a = (lon * PI) / 180.0, b = (lat * PI) / 180.0;
    if (mode == 0) {
        out[2 * i + 0] = a;
        out[2 * i + 1] = b;
    } else {
        const double cb = cos(b);
        out[3 * i + 0] = cb * cos(a);
        out[3 * i + 1] = cb * sin(a);
        out[3 * i + 2] = sin(b);
    }
}
