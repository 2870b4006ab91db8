/* ref_host.h -- forced-include header (g++ -include) that lets the reference's CUDA translation units compile for the
 * host, unchanged but for their launches (oracle/reference.py rewrites `k<<<grid, block, 0, stream>>>(args)` into
 * `ref_launch(k, Dim3{grid}, Dim3{block}, args)`).
 *
 * TEST INFRASTRUCTURE, like everything under oracle/. Written from scratch; it quotes nothing of the reference.
 *
 * A "launch" here is a serial loop over blocks and threads in the calling thread, with blockIdx / threadIdx / blockDim
 * as plain globals: right for kernels that are pure per-thread functions of their indices (no shared memory, no
 * barriers, no atomics - reference.py checks the source for them) and for ONE caller at a time. The module built with
 * this header is single-threaded by construction. */
#pragma once
#include <torch/extension.h>            /* all of ATen and pybind11 BEFORE the renames below */
#include <cmath>
#include <cstring>

/* device tensors become host tensors (after ATen is in, so that only the reference's own text is renamed) */
#define kCUDA kCPU
#define is_cuda is_cpu

#define __global__
#define __device__
#define __host__
#define __constant__

typedef unsigned int uint;
using std::isnan;

struct Dim3 {
    unsigned x, y, z;
    Dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
static Dim3 blockIdx, threadIdx, blockDim, gridDim;

template <class Symbol>
inline int cudaMemcpyToSymbol(Symbol& symbol, const void* src, size_t bytes) { std::memcpy(&symbol, src, bytes); return 0; }

/* sin(pi x), cos(pi x) for CUDA's sinpif / cospif, which this libm lacks. Independent of the oracle's or_sincospi
 * (Taylor series in double): fmodf(x, 2) is exact; the fold to the nearest quarter turn is exact in double (a binary32
 * value minus a multiple of 1/2), so quarter turns give exact 0 and +-1 as CUDA's do; then libm's double sin / cos of
 * M_PI*z for |z| <= 1/4, rounded to binary32 once. */
static inline void ref_sincospi(float x, float* s, float* c) {
    const double y = (double)std::fmod(x, 2.f);
    const double k = std::nearbyint(2.*y);
    const double z = y - .5*k;
    const double S = std::sin(M_PI*z), C = std::cos(M_PI*z);
    switch (((int)k) & 3) {
        case 0:  *s = (float)S;    *c = (float)C;    break;
        case 1:  *s = (float)C;    *c = (float)(-S); break;
        case 2:  *s = (float)(-S); *c = (float)(-C); break;
        default: *s = (float)(-C); *c = (float)S;    break;
    }
}
static inline float sinpif(float x) { float s, c; ref_sincospi(x, &s, &c); return s; }
static inline float cospif(float x) { float s, c; ref_sincospi(x, &s, &c); return c; }

#ifdef REF_EXPORT_SINCOSPI              /* one translation unit exports them for the tests' sweep (ctypes) */
extern "C" __attribute__((visibility("default"))) float ref_sinpif(float x) { return sinpif(x); }
extern "C" __attribute__((visibility("default"))) float ref_cospif(float x) { return cospif(x); }
extern "C" __attribute__((visibility("default"))) void ref_sincospi_many(const float* x, float* s, float* c, long n) {
    for (long i = 0; i < n; i++) ref_sincospi(x[i], s + i, c + i);
}
#endif

template <typename Kernel, typename... Args>
inline void ref_launch(Kernel kernel, Dim3 grid, Dim3 block, Args... args) {
    gridDim = grid; blockDim = block;
    for (unsigned bz = 0; bz < grid.z; bz++) for (unsigned by = 0; by < grid.y; by++) for (unsigned bx = 0; bx < grid.x; bx++)
    for (unsigned tz = 0; tz < block.z; tz++) for (unsigned ty = 0; ty < block.y; ty++) for (unsigned tx = 0; tx < block.x; tx++) {
        blockIdx = Dim3(bx, by, bz); threadIdx = Dim3(tx, ty, tz);
        kernel(args...);
    }
}
