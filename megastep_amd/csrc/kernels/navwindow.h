// kernels/navwindow.h -- nav_window_kernel.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, after navseen.h; an
// env's grid is navfield.h's NavCells, the store a view reads its nav_layer_store); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// map windows: per-cell stores cropped and turned into images round each agent      no counterpart in the reference
// ------------------------------------------------------------------------------------------------
// The contract is written out in include/megastep_hip.h (MsNavWindows) and DESIGN.md section 3.18: a pixel's k*k sub-samples
// go through the view's affine map to world points; the cell under each is found as the seen maps find it; a channel reads a
// byte or a float store at that cell, behind an optional gate; the pixel is the serial mean of the k*k values.  Every output
// element has one writer and a fixed serial sum, so nothing depends on the order of execution.
// tests/test_navwindow_host.py restates all of it in numpy (window_rule).
//
// The rule's pieces - win_point, win_cell, win_byte, win_float, win_pixel - are __host__ __device__ functions over
// plain numbers: ms_host_nav_windows runs them on host arrays, so the CPU suite holds this very text to window_rule, bit for bit.
//
//   nav_window_kernel<K>   one launch for every image and every channel; K = samples, so that the K*K cells of a pixel are
//                     registers (an array indexed by unrolled loops only: no scratch).  blockIdx.x is the image (n, p),
//                     blockIdx.y a run of WG pixels of its flattened row-major H*W: a lane owns a pixel, a wave's store to a
//                     channel plane is 256 contiguous bytes except at the image's end, and a 16 x 16 image fills its
//                     workgroup.  Everything that is the same for an image - the env's geom and first cell, the six view
//                     floats, each channel's descriptor (kernel arguments, by value), field indices and store bases - hangs
//                     on blockIdx alone and is read through scalar loads.  The cells are computed once and shared by the
//                     channels; the byte and float gathers go straight to global memory (a window's footprint is a few KiB
//                     and stays in L2 from step to step).  No LDS, no atomics, no barrier.
constexpr int WIN_MAX_CHANNELS = 8, WIN_MAX_SAMPLES = 4, WIN_MAX_SIDE = 1024;

struct WinView { float g0, g1, g2, g3, g4, g5; };

struct WinChannel {                                  // MsNavChannel, checked
    const void* source;                              // bytes or floats: n_fields stores per env
    const int* source_field;                         // (N, P) or NULL
    const unsigned char* gate;                       // bytes, or NULL: no gate
    const int* gate_field;                           // (N, P) or NULL
    int source_fields, gate_fields;
    int is_float, where;
    float scale, outside, hidden;
};

struct NavWindowArgs {                               // MsNavWindows, checked
    const float* views;                              // (N, P, 6)
    float* out;                                      // (N, P, C, H, W)
    int n_views, height, width, n_channels;
    WinChannel ch[WIN_MAX_CHANNELS];
};

// Sub-sample (a, b) of pixel (row i from the top, column j) at k samples a side, through view g.
__host__ __device__ inline void win_point(const WinView& g, const int i, const int j, const int a, const int b, const int k, float& x, float& y) {
    const float u = (float)j + ((float)b + .5f)/(float)k;
    const float w = (float)i + ((float)a + .5f)/(float)k;
    x = (g.g0*u + g.g1*w) + g.g2;
    y = (g.g3*u + g.g4*w) + g.g5;
}

// The cell under (x, y), row-major in its env's grid; -1: none (seen_sample's statements).
__host__ __device__ inline long long win_cell(const NavCells& g, const float x, const float y) {
    const float fx = floorf(x/g.c), fy = floorf(y/g.c);
    if (!(fabsf(fx) < NAV_INDEX_LIMIT) || !(fabsf(fy) < NAV_INDEX_LIMIT)) return -1;
    const long long j = (long long)(int)fx - g.jx0, i = (long long)(int)fy - g.iy0;   // (|fx|, |fy| < 2^30: the int holds them)
    if ((i < 0) | (i >= g.ny) | (j < 0) | (j >= g.nx)) return -1;
    return i*g.nx + j;
}

__host__ __device__ inline float win_byte(const unsigned char byte, const int where) { return (byte != 0) == (where != 0) ? 1.f : 0.f; }

__host__ __device__ inline float win_float(const float D, const float scale) {
    const float v = D*scale;
    return v < 1.f ? (v > 0.f ? v : 0.f) : 1.f;      // (a NaN is not < 1: 1)
}

// One pixel of one channel from the pixel's K*K cells: `source` and `gate` are the stores the view reads (gate NULL: none).
template <int K>
__host__ __device__ inline float win_pixel(const WinChannel& ch, const void* source, const unsigned char* gate, const long long (&cell)[K*K]) {
    float acc = 0.f;
#pragma unroll
    for (int s = 0; s < K*K; s++) {
        const long long at = cell[s];
        float v = ch.outside;
        if (at >= 0) {
            if (gate && gate[at] == 0) v = ch.hidden;
            else if (ch.is_float) v = win_float(static_cast<const float*>(source)[at], ch.scale);
            else v = win_byte(static_cast<const unsigned char*>(source)[at], ch.where);
        }
        acc += v;
    }
    return acc/(float)(K*K);
}

// One pixel of every channel: out points at the pixel in the image's first plane, planes hw apart.
template <int K>
__host__ __device__ inline void win_pixels(const NavCells& g, const long long first, const WinView& view, const NavWindowArgs& q,
                                           const long long image, const int p, const int i, const int j, const long long hw, float* out) {
    const long long cells = g.nx > 0 && g.ny > 0 ? (long long)g.nx*g.ny : 0;
    long long cell[K*K];
#pragma unroll
    for (int a = 0; a < K; a++) {
#pragma unroll
        for (int b = 0; b < K; b++) {
            float x, y;
            win_point(view, i, j, a, b, K, x, y);
            cell[a*K + b] = win_cell(g, x, y);
        }
    }
    for (int c = 0; c < q.n_channels; c++) {
        const WinChannel& ch = q.ch[c];
        const int fs = nav_layer_store(ch.source_field, ch.source_fields, image, p);
        const int fg = ch.gate ? nav_layer_store(ch.gate_field, ch.gate_fields, image, p) : 0;
        float v;
        if (fs < 0) v = ch.outside;
        else if (fg < 0) v = ch.hidden;
        else {
            const long long at = (long long)ch.source_fields*first + (long long)fs*cells;
            const void* const source = ch.is_float ? static_cast<const void*>(static_cast<const float*>(ch.source) + at)
                                                   : static_cast<const void*>(static_cast<const unsigned char*>(ch.source) + at);
            const unsigned char* const gate = ch.gate ? ch.gate + ((long long)ch.gate_fields*first + (long long)fg*cells) : nullptr;
            v = win_pixel<K>(ch, source, gate, cell);
        }
        out[c*hw] = v;
    }
}

// One call, serially (host instantiation only).
template <int K>
inline void win_serial(const NavArgs& a, const NavWindowArgs& q) {
    const long long hw = (long long)q.height*q.width;
    for (long long image = 0; image < (long long)a.n_envs*q.n_views; image++) {
        const int e = (int)(image / q.n_views), p = (int)(image - (long long)e*q.n_views);
        const NavCells g = nav_cells(a, e);
        const float* const v = q.views + image*6;
        const WinView view{v[0], v[1], v[2], v[3], v[4], v[5]};
        for (int i = 0; i < q.height; i++)
            for (int j = 0; j < q.width; j++)
                win_pixels<K>(g, a.starts[e], view, q, image, p, i, j, hw, q.out + image*q.n_channels*hw + (long long)i*q.width + j);
    }
}

template <int K>
__global__ __launch_bounds__(WG) void nav_window_kernel(const NavArgs a, const NavWindowArgs q) {
    const unsigned image = blockIdx.x;                                  // (n, p): n P + p
    const int hw = q.height*q.width;                                    // (at most 2^20)
    const int px = (int)blockIdx.y*WG + (int)threadIdx.x;               // the lane's pixel of the flattened image
    if (px >= hw) return;
    const int e = (int)(image / (unsigned)q.n_views), p = (int)(image - (unsigned)e*(unsigned)q.n_views);
    const int4 geom = reinterpret_cast<const int4*>(a.geom)[e];
    const NavCells g{geom.x, geom.y, geom.z, geom.w, a.cell};
    const float* const v = q.views + (long long)image*6;
    const WinView view{v[0], v[1], v[2], v[3], v[4], v[5]};
    const int i = px / q.width, j = px - i*q.width;
    win_pixels<K>(g, a.starts[e], view, q, image, p, i, j, hw, q.out + (long long)image*q.n_channels*hw + px);
}
