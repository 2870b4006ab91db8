// kernels/overhead.h -- overhead_kernel.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, after render.h: it uses
// render.h's drawn_row for the agents' rows); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// top-down pictures of the envs                        no counterpart as a kernel (reference: plotting.py, matplotlib)
// ------------------------------------------------------------------------------------------------
// Image k shows env envs[k] through V views; view g maps pixel centres to world metres by an affine map (six floats).  A
// pixel takes the colour of the nearest line within the half width h of its centre (ties: the lower line index), the
// caller's background where there is none.  The rule is written out in include/megastep_hip.h (MsOverhead) and in
// DESIGN.md section 3.13; every operation is one binary32 operation, so tests/test_overhead_host.py restates it in numpy
// bit for bit.
//
// One 256-lane workgroup per 16 x 16 tile of one image: env, view and line rows are the same for the whole block.
//   pass 1 (cull)  the block's lanes test the env's lines 256 at a time against the tile's footprint - the box of the
//                  tile's pixel centres grown by h and by slack for rounding - and compact the survivors into LDS;
//   pass 2 (fold)  each lane folds its pixel over the LDS list by (d2, index): the order of the list does not matter;
//   chunking       when the list could overflow its OV_CHUNK rows, the block folds it, empties it and culls on, the
//                  pixels' best (d2, index, t) carried in registers;
//   epilogue       the winner's texel and the stores, lanes outside the image masked.
constexpr int OV_TILE = 16;                 // tile side: OV_TILE^2 = WG pixels, one per lane
constexpr int OV_CHUNK = 1024;              // line rows the LDS list holds (16 KB of rows + 4 KB of indices)
static_assert(OV_TILE*OV_TILE == WG, "one pixel per lane");
static_assert(OV_CHUNK % WG == 0 && OV_CHUNK >= 2*WG, "a window of WG lines must fit after a partly filled list");

// The launch's arguments (ms_overhead's MsOverhead, checked, plus the launch's place in the whole job).
struct OvArgs {
    const int* envs;                        // (K,) or NULL: image k shows env k
    const float* views;                     // (K, V, 6)
    float* rgb;                             // (K, V, 3, H, W) or NULL
    int* indices;                           // (K, V, H, W) or NULL
    long long block0;                       // first (image, view, tile) block of this launch
    int n_views, height, width, tiles_x, tiles_y;
    float half_width, h2;                   // h and h*h (binary32, as the rule squares it)
    float bg_r, bg_g, bg_b;
    int lit, with_agents, cull;
};

// The tile's footprint: the box of the pixel centres of rows i0..i1 and columns j0..j1 under view g.  The view is affine,
// so the exact images of all the tile's centres lie in the box of its four corners' images; each computed coordinate is
// off its exact value by at most 3 ulps of |g0 u| + |g1 w| + |g2| (three roundings), which `slack` (1e-5 of that, some 170
// ulps) covers twice over.  `mag`: the largest coordinate of the box, for the line test's own slack.  Not finite: no cull.
struct OvBox { float x0, y0, x1, y1, mag; bool finite; };

__host__ __device__ inline OvBox ov_footprint(const float g0, const float g1, const float g2, const float g3, const float g4,
                                              const float g5, const int i0, const int j0, const int i1, const int j1) {
    const float ua = (float)j0 + .5f, ub = (float)j1 + .5f, wa = (float)i0 + .5f, wb = (float)i1 + .5f;
    const float xs[4] = {(g0*ua + g1*wa) + g2, (g0*ub + g1*wa) + g2, (g0*ua + g1*wb) + g2, (g0*ub + g1*wb) + g2};
    const float ys[4] = {(g3*ua + g4*wa) + g5, (g3*ub + g4*wa) + g5, (g3*ua + g4*wb) + g5, (g3*ub + g4*wb) + g5};
    OvBox b{xs[0], ys[0], xs[0], ys[0], 0.f, true};
    for (int c = 0; c < 4; c++) {
        b.finite = b.finite && isfinite(xs[c]) && isfinite(ys[c]);
        b.x0 = fminf(b.x0, xs[c]); b.x1 = fmaxf(b.x1, xs[c]);
        b.y0 = fminf(b.y0, ys[c]); b.y1 = fmaxf(b.y1, ys[c]);
    }
    const float sx = 1e-5f*((fabsf(g0)*ub + fabsf(g1)*wb) + fabsf(g2));
    const float sy = 1e-5f*((fabsf(g3)*ub + fabsf(g4)*wb) + fabsf(g5));
    b.finite = b.finite && isfinite(sx) && isfinite(sy);
    b.x0 -= sx; b.x1 += sx; b.y0 -= sy; b.y1 += sy;
    b.mag = fmaxf(fmaxf(fabsf(b.x0), fabsf(b.x1)), fmaxf(fabsf(b.y0), fabsf(b.y1)));
    return b;
}

// Can line L = (ax, ay, bx, by) cover a pixel whose centre lies in box b, at half width h?  False only when it cannot.
// The rule's computed d2 is within a few ulps of the squared distance from the centre to a point of the exact segment (its
// t is clamped into [0, 1]) give or take a few ulps of the coordinates: d2 <= h*h puts the centre within
// r = h + 1e-5 (h + |coordinates|) of the segment, r far above those ulps.  The segment is then tested against the box
// grown by r - which holds every point within r of the box - by its bounding box and by the separating axis along its
// normal, with slack of its own for the roundings of that test.  (A line with a NaN or an infinity in its row never
// covers: its d2 is NaN.  The cull may drop it or keep it.)
__host__ __device__ inline bool ov_keeps(const OvBox& b, const float h, const float4 L) {
    if (!b.finite) return true;
    const float mag = fmaxf(fmaxf(fabsf(L.x), fabsf(L.y)), fmaxf(fabsf(L.z), fabsf(L.w)));
    const float r = h + 1e-5f*(h + mag + b.mag);
    const float x0 = b.x0 - r, x1 = b.x1 + r, y0 = b.y0 - r, y1 = b.y1 + r;
    if ((fmaxf(L.x, L.z) < x0) || (fminf(L.x, L.z) > x1) || (fmaxf(L.y, L.w) < y0) || (fminf(L.y, L.w) > y1)) return false;
    const float vx = L.z - L.x, vy = L.w - L.y;
    const float cx = .5f*(x0 + x1), cy = .5f*(y0 + y1), ex = .5f*(x1 - x0), ey = .5f*(y1 - y0);
    const float qx = cx - L.x, qy = cy - L.y;
    const float sep = fabsf(vx*qy - vy*qx);
    const float reach = ex*fabsf(vy) + ey*fabsf(vx);
    const float tol = 1e-5f*(fabsf(vx) + fabsf(vy))*(fabsf(qx) + fabsf(qy) + ex + ey + fabsf(vx) + fabsf(vy));
    return !(sep > reach + tol);
}

// A pixel's best line so far: least d2, then least index (INT_MAX: none).
struct OvBest { float d2; int idx; float t; };

// One line of the rule for the pixel centre (x, y): statement for statement include/megastep_hip.h's MsOverhead.
__host__ __device__ inline void ov_fold(const float x, const float y, const float4 L, const int l, const float h2, OvBest& b) {
    const float vx = L.z - L.x, vy = L.w - L.y, px = x - L.x, py = y - L.y;
    const float vv = vx*vx + vy*vy;
    float t = vv > 0.f ? (px*vx + py*vy)/vv : 0.f;
    t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);                           // (a NaN stays NaN)
    const float dx = px - t*vx, dy = py - t*vy;
    const float d2 = dx*dx + dy*dy;
    if ((d2 <= h2) & ((d2 < b.d2) | ((d2 == b.d2) & (l < b.idx)))) { b.d2 = d2; b.idx = l; b.t = t; }
}

__global__ __launch_bounds__(WG) void overhead_kernel(const MsScenery sc, const AgentsK ag, const OvArgs a) {
    __shared__ float4 s_rows[OV_CHUNK];
    __shared__ int s_idx[OV_CHUNK];
    __shared__ int s_wave[WAVES];
    const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE;
    const long long blk = a.block0 + blockIdx.x;
    const int tiles = a.tiles_x*a.tiles_y;
    const long long kv = blk / tiles;                                   // image k, view v: k V + v
    const int tile = (int)(blk - kv*tiles);
    const int k = (int)(kv / a.n_views);
    const int ty = tile / a.tiles_x, tx = tile - ty*a.tiles_x;
    const int i0 = ty*OV_TILE, j0 = tx*OV_TILE;
    const int i = i0 + tid / OV_TILE, j = j0 + tid % OV_TILE;
    const bool live = (i < a.height) & (j < a.width);
    const long long hw = (long long)a.height*a.width;
    const long long at = kv*hw + (long long)i*a.width + j;              // (K, V, H, W) offset of the lane's pixel
    const int e = __builtin_amdgcn_readfirstlane(a.envs ? a.envs[k] : k);

    OvBest best{INFINITY, INT_MAX, 0.f};
    int base = 0, AF = 0;
    if ((e >= 0) & (e < sc.n_envs)) {                                   // (an env id out of range: background, nothing read)
        const float* const g = a.views + kv*6;
        const float g0 = g[0], g1 = g[1], g2 = g[2], g3 = g[3], g4 = g[4], g5 = g[5];
        const float u = (float)j + .5f, w = (float)i + .5f;
        const float x = (g0*u + g1*w) + g2, y = (g3*u + g4*w) + g5;
        const OvBox box = ov_footprint(g0, g1, g2, g3, g4, g5, i0, j0, min(i0 + OV_TILE - 1, a.height - 1),
                                       min(j0 + OV_TILE - 1, a.width - 1));
        const int L = sc.lines_widths[e];
        base = sc.lines_starts[e];
        const int A = sc.n_agents, M = sc.n_model;
        AF = A*M;
        const float4* const rows = reinterpret_cast<const float4*>(sc.lines_vals) + base;
        int count = 0;
        for (int l0 = 0; l0 < L; l0 += WG) {
            const int l = l0 + tid;
            bool keep = false;
            float4 row = make_float4(0.f, 0.f, 0.f, 0.f);
            if (l < L) {
                if (a.with_agents && l < AF) {                          // the agent's row at its current pose, as ms_render draws it
                    const int agent = l / M;
                    float s, c;
                    sincospi_f(ag.angles[e*A + agent]/180.f, s, c);
                    const float2 p = reinterpret_cast<const float2*>(ag.positions)[e*A + agent];
                    row = drawn_row(s, c, p.x, p.y, reinterpret_cast<const float4*>(sc.model)[l - agent*M]);
                } else {
                    row = rows[l];
                }
                keep = !a.cull || ov_keeps(box, a.half_width, row);
            }
            // compaction: the wave's survivors by ballot, the waves' counts through LDS
            const unsigned long long m = __ballot(keep);
            if (lane == 0) s_wave[wave] = (int)__popcll(m);
            __syncthreads();
            int off = count, total = 0;
            for (int q = 0; q < WAVES; q++) {
                const int c = s_wave[q];
                off += q < wave ? c : 0;
                total += c;
            }
            off += (int)__popcll(m & ((1ull << lane) - 1ull));
            if (keep) { s_rows[off] = row; s_idx[off] = l; }
            count += total;
            __syncthreads();
            if (count > OV_CHUNK - WG || l0 + WG >= L) {                // (uniform) the list is full, or the env's lines are done
                for (int q = 0; q < count; q++) ov_fold(x, y, s_rows[q], s_idx[q], a.h2, best);
                count = 0;
                __syncthreads();
            }
        }
    }

    if (!live) return;
    float r = a.bg_r, gr = a.bg_g, bl = a.bg_b;
    int idx = -1;
    if (best.idx != INT_MAX) {
        idx = best.idx;
        r = gr = bl = 0.f;                                              // (a line without texels)
        const int gl = base + idx;
        const int tw = a.rgb ? sc.textures_widths[gl] : 0;
        if (tw > 0) {
            const int q = min((int)(best.t*(float)tw), tw - 1);
            const long long tex = (long long)sc.textures_starts[gl] + q;
            r = sc.textures_vals[3*tex]; gr = sc.textures_vals[3*tex + 1]; bl = sc.textures_vals[3*tex + 2];
            if (a.lit && idx >= AF) {
                const float bk = sc.baked_vals[tex];
                r = r*bk; gr = gr*bk; bl = bl*bk;
            }
        }
    }
    if (a.indices) a.indices[at] = idx;
    if (a.rgb) {
        const long long px = kv*3*hw + (long long)i*a.width + j;
        a.rgb[px] = r; a.rgb[px + hw] = gr; a.rgb[px + 2*hw] = bl;
    }
}
