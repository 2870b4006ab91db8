// kernels/navview.h -- nav_view_kernel.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, after navregion.h: a cell's
// centre is navfield.h's nav_centre); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// view fields: the cells in sight of a point, and how much of it is new   no counterpart in the reference
// ------------------------------------------------------------------------------------------------
// The contract is written out in include/megastep_hip.h (MsNavViews) and DESIGN.md section 3.21: a cell is visible from a
// viewpoint when its centre is in range, in the cone if one is given, and no static wall of the env blocks the segment between
// the two - a wall blocks when its box meets the segment's, the two ends of the segment lie strictly on opposite sides of its
// line, and its own ends lie on opposite sides (zero included) of the segment's.  A cell's value is an OR over the walls of a
// pure predicate, every output a byte with one writer or an integer count: any wall order, any cull consistent with `meets`
// and any schedule give the same result.  tests/test_navview_host.py restates all of it in numpy (view_rule).
//
// The rule's pieces - view_in_range, view_in_cone, view_wall_blocks, view_window, view_keeps, view_tile_box - are __host__ __device__ functions
// over plain numbers: ms_host_nav_views sweeps them serially over host arrays, through the kernel's own window, cull and both
// wall paths, so the CPU suite holds this very text to view_rule, byte for byte.
//
//   nav_view_kernel   one WORKGROUP a viewpoint (n, p).  The window: the rows and columns whose centres can be in range; the
//                     bytes of the store outside it are written 0.  The env's static rows are read WG at a time, a row kept
//                     when its box meets the box of everything in range, and the kept rows compacted into LDS by ballot and
//                     prefix count (VIEW_WALL_CAPACITY rows; more than fit: the viewpoint sweeps the env's rows in global memory
//                     at wave-uniform addresses instead, to the same bits).  A wave takes tiles of 8 x 8 window cells, a lane a
//                     cell, and walks the walls at a wave-uniform index (LDS broadcasts) until every lane is blocked, passing
//                     over - for four comparisons - a wall whose box misses the box of the tile and the viewpoint: it fails
//                     `meets` for every cell of the tile.  Then the bytes are stored and the ballots visible & countable
//                     (& !seen) counted.  The counts go
//                     through LDS across the waves; one lane stores them.  No atomics, no scratch; with values == NULL no
//                     byte is written at all - scoring candidate standpoints needs no store.
constexpr int VIEW_WALL_CAPACITY = 512;              // rows of four floats staged in LDS, 8 KiB: every wall of a plan of the headline's kind

struct ViewPoint { float px, py, hx, hy, hlen; bool cone; };
struct ViewWindow { int i0, i1, j0, j1; };           // rows i0 .. i1 - 1, columns j0 .. j1 - 1
struct ViewBox { float x0, y0, x1, y1; };            // p -+ R1: holds every in-range centre

// The viewpoint as the cells read it; false: it sees nothing (a NaN or infinite point; with a cone, a heading without a length).
__host__ __device__ inline bool view_point(const float px, const float py, const bool cone, const float hx, const float hy, ViewPoint& v) {
    v.px = px; v.py = py; v.hx = 0.f; v.hy = 0.f; v.hlen = 0.f; v.cone = cone;
    if (!(nav_finite(px) && nav_finite(py))) return false;
    if (!cone) return true;
    v.hx = hx; v.hy = hy;
    v.hlen = sqrtf(v.hx*v.hx + v.hy*v.hy);
    return nav_finite(v.hlen) && v.hlen > 0.f;
}

__host__ __device__ inline bool view_in_range(const float rr, const float R2) { return rr <= R2; }

__host__ __device__ inline bool view_in_cone(const ViewPoint& v, const float rx, const float ry, const float rr, const float cos_half) {
    const float len = sqrtf(rr);
    const float dotp = v.hx*rx + v.hy*ry;
    const float lim = (cos_half*len)*v.hlen;
    return dotp >= lim;
}

// Does wall w = (ax, ay, bx, by) block the segment from (px, py) to the centre (x, y); (rx, ry) = (x - px, y - py).  The four
// comparisons of `meets` first, the cross products only behind them.  A NaN in the wall fails `apart`, whatever `meets` made of it.
__host__ __device__ inline bool view_wall_blocks(const float px, const float py, const float x, const float y, const float rx, const float ry,
                                                 const float4 w) {
    const float wx0 = w.x < w.z ? w.x : w.z, wx1 = w.x > w.z ? w.x : w.z, wy0 = w.y < w.w ? w.y : w.w, wy1 = w.y > w.w ? w.y : w.w;
    const float sx0 = px < x ? px : x, sx1 = px > x ? px : x, sy0 = py < y ? py : y, sy1 = py > y ? py : y;
    if (!((wx0 <= sx1) & (wx1 >= sx0) & (wy0 <= sy1) & (wy1 >= sy0))) return false;
    const float vx = w.z - w.x, vy = w.w - w.y;
    const float o1 = vx*(py - w.y) - vy*(px - w.x);
    const float o2 = vx*(y - w.y) - vy*(x - w.x);
    if (!(((o1 < 0.f) & (o2 > 0.f)) | ((o1 > 0.f) & (o2 < 0.f)))) return false;
    const float o3 = rx*(w.y - py) - ry*(w.x - px);
    const float o4 = rx*(w.w - py) - ry*(w.z - px);
    return ((o3 <= 0.f) & (o4 >= 0.f)) | ((o3 >= 0.f) & (o4 <= 0.f));
}

// The indices lo .. hi - 1 of the n cells from `origin` on whose centres can lie within R of p on this axis.  An in-range
// centre x has |x - p| <= R(1 + 2^-22); x, the binary32 ((float)k + .5f)*c, lies within 1.51 cells of (k + .5)c for |k| up to
// 2^24 + 2^15; so k is no further than two cells beyond floor((p -+ R 1.000001)/c), here in binary64.
__host__ __device__ inline void view_span(const float p, const float R, const float c, const int origin, const int n, int& lo, int& hi) {
    const double reach = (double)R*1.000001;
    const double a = floor(((double)p - reach)/(double)c) - 2. - (double)origin;
    const double b = floor(((double)p + reach)/(double)c) + 2. - (double)origin;
    lo = a < 0. ? 0 : a > (double)n ? n : (int)a;
    hi = b < 0. ? 0 : b >= (double)(n - 1) ? n : (int)b + 1;
    if (hi < lo) hi = lo;
}

__host__ __device__ inline ViewWindow view_window(const ViewPoint& v, const float R, const float c, const int jx0, const int iy0, const int nx, const int ny) {
    ViewWindow w;
    view_span(v.py, R, c, iy0, ny, w.i0, w.i1);
    view_span(v.px, R, c, jx0, nx, w.j0, w.j1);
    return w;
}

// The box of everything in range: an in-range centre x has |x - p| <= R(1 + 2^-22) < R1 = R*1.0001f + c, and rounding is monotone,
// so fl(p - R1) <= min(p, x) and fl(p + R1) >= max(p, x): a wall whose box misses this one fails `meets` for every in-range cell.
__host__ __device__ inline ViewBox view_box(const ViewPoint& v, const float R, const float c) {
    const float R1 = R*1.0001f + c;
    return ViewBox{v.px - R1, v.py - R1, v.px + R1, v.py + R1};
}
__host__ __device__ inline bool view_keeps(const ViewBox& b, const float4 w) {
    const float wx0 = w.x < w.z ? w.x : w.z, wx1 = w.x > w.z ? w.x : w.z, wy0 = w.y < w.w ? w.y : w.w, wy1 = w.y > w.w ? w.y : w.w;
    return (wx0 <= b.x1) & (wx1 >= b.x0) & (wy0 <= b.y1) & (wy1 >= b.y0);
}

// The box of a tile of cells and the viewpoint: centres are monotone in the index, so it holds the segment to every cell whose
// centre lies between (xa, ya) and (xb, yb); a wall whose box misses it fails `meets` for every cell of the tile.
constexpr int VIEW_TILE = 8;                         // a wave's cells: 8 x 8
__host__ __device__ inline ViewBox view_tile_box(const ViewPoint& v, const float xa, const float ya, const float xb, const float yb) {
    return ViewBox{v.px < xa ? v.px : xa, v.py < ya ? v.py : ya, v.px > xb ? v.px : xb, v.py > yb ? v.py : yb};
}

struct NavViewArgs {                                 // MsNavViews, checked
    const float* points;                             // (N, P, 2)
    const float* headings;                           // (N, P, 2) or NULL
    const unsigned char* mask;                       // (N, P) or NULL
    const unsigned char* countable;                  // (starts[N],)
    const unsigned char* unseen;                     // S*starts[N] bytes or NULL
    const int* slot;                                 // (N, P) or NULL
    unsigned char* values;                           // P*starts[N] bytes or NULL
    int* counts;                                     // (N, P) or NULL
    int* gains;                                      // (N, P) or NULL
    int n_points, n_maps, capacity;
    float R, R2, cos_half;
};

// The map viewpoint (n, p) reads its gains against: -1 none (no maps asked for, or a slot outside 0 .. S - 1).
__host__ __device__ inline int view_slot(const NavViewArgs& q, const long long vp, const int p) {
    if (!q.unseen || !q.gains) return -1;
    return nav_layer_store(q.slot, q.n_maps, vp, p);
}

// One cell of the window against the walls given: is it in sight?  (host: the serial sweep's inner loop)
__host__ __device__ inline bool view_candidate(const ViewPoint& v, const float x, const float y, const float R2, const float cos_half, float& rx, float& ry) {
    rx = x - v.px; ry = y - v.py;
    const float rr = rx*rx + ry*ry;
    return view_in_range(rr, R2) && (!v.cone || view_in_cone(v, rx, ry, rr, cos_half));
}

// One whole call on host arrays, serially: `walls` holds every env's STATIC rows, env n's from wall_starts[n] on.
inline void view_serial(const NavArgs& a, const NavViewArgs& q, const float4* walls, const long long* wall_starts) {
    std::vector<float4> staged((size_t)(q.capacity > 0 ? q.capacity : 1));
    for (int e = 0; e < a.n_envs; e++)
        for (int p = 0; p < q.n_points; p++) {
            const long long vp = (long long)e*q.n_points + p;
            if (q.mask && !q.mask[vp]) continue;
            const NavCells g = nav_cells(a, e);
            const int jx0 = g.jx0, iy0 = g.iy0, nx = g.nx, ny = g.ny;
            const long long cells = nx > 0 && ny > 0 ? (long long)nx*ny : 0;
            if (cells <= 0) {
                if (q.counts) q.counts[vp] = 0;
                if (q.gains) q.gains[vp] = 0;
                continue;
            }
            ViewPoint v;
            const bool live = view_point(q.points[2*vp], q.points[2*vp + 1], q.headings != nullptr, q.headings ? q.headings[2*vp] : 0.f,
                                         q.headings ? q.headings[2*vp + 1] : 0.f, v);
            ViewWindow w{0, 0, 0, 0};
            if (live) w = view_window(v, q.R, a.cell, jx0, iy0, nx, ny);
            const int s = view_slot(q, vp, p);
            const unsigned char* const seen = s >= 0 ? q.unseen + (long long)q.n_maps*a.starts[e] + (long long)s*cells : nullptr;
            const unsigned char* const counts = q.countable + a.starts[e];
            unsigned char* const out = q.values ? q.values + (long long)q.n_points*a.starts[e] + (long long)p*cells : nullptr;
            const float4* const rows = walls + wall_starts[e];
            const long long n_rows = wall_starts[e + 1] - wall_starts[e];
            long long kept = 0;
            if (w.i1 > w.i0 && w.j1 > w.j0) {
                const ViewBox box = view_box(v, q.R, a.cell);
                for (long long l = 0; l < n_rows; l++)
                    if (view_keeps(box, rows[l])) {
                        if (kept < q.capacity) staged[(size_t)kept] = rows[l];
                        kept++;
                    }
            }
            const bool overflow = kept > q.capacity;
            int count = 0, gain = 0;
            for (int i = 0; i < ny; i++)
                for (int j = 0; j < nx; j++) {
                    const long long cell = (long long)i*nx + j;
                    bool visible = false;
                    if (i >= w.i0 && i < w.i1 && j >= w.j0 && j < w.j1) {
                        const float x = nav_centre(jx0, j, a.cell), y = nav_centre(iy0, i, a.cell);
                        const int ia = w.i0 + (i - w.i0)/VIEW_TILE*VIEW_TILE, ja = w.j0 + (j - w.j0)/VIEW_TILE*VIEW_TILE;      // the cell's tile
                        const int ib = ia + VIEW_TILE - 1 < w.i1 - 1 ? ia + VIEW_TILE - 1 : w.i1 - 1, jb = ja + VIEW_TILE - 1 < w.j1 - 1 ? ja + VIEW_TILE - 1 : w.j1 - 1;
                        const ViewBox tile = view_tile_box(v, nav_centre(jx0, ja, a.cell), nav_centre(iy0, ia, a.cell), nav_centre(jx0, jb, a.cell),
                                                           nav_centre(iy0, ib, a.cell));
                        float rx, ry;
                        visible = view_candidate(v, x, y, q.R2, q.cos_half, rx, ry);
                        if (!overflow)
                            for (long long k = 0; k < kept && visible; k++)
                                visible = !(view_keeps(tile, staged[(size_t)k]) && view_wall_blocks(v.px, v.py, x, y, rx, ry, staged[(size_t)k]));
                        else
                            for (long long l = 0; l < n_rows && visible; l++)
                                visible = !(view_keeps(tile, rows[l]) && view_wall_blocks(v.px, v.py, x, y, rx, ry, rows[l]));
                    }
                    if (out) out[cell] = visible ? 1 : 0;
                    const bool counted = visible && (counts[cell] & 1);
                    count += counted;
                    gain += counted && seen && !(seen[cell] & 1);
                }
            if (q.counts) q.counts[vp] = count;
            if (q.gains) q.gains[vp] = gain;
        }
}

__global__ __launch_bounds__(WG) void nav_view_kernel(const MsScenery sc, const NavArgs a, const NavViewArgs q) {
    __shared__ float4 s_walls[VIEW_WALL_CAPACITY];
    __shared__ int s_kept[WAVES], s_count[WAVES], s_gain[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long vp = blockIdx.x;                                    // (n, p): n P + p
    const int e = (int)(vp / q.n_points), p = (int)(vp - (long long)e*q.n_points);
    if (q.mask && !q.mask[vp]) return;                                  // (uniform)
    const int4 geom = reinterpret_cast<const int4*>(a.geom)[e];
    const int nx = geom.z, ny = geom.w;
    const long long cells = nx > 0 && ny > 0 ? (long long)nx*ny : 0;
    if (cells <= 0) {                                                   // (uniform)
        if (tid == 0) {
            if (q.counts) q.counts[vp] = 0;
            if (q.gains) q.gains[vp] = 0;
        }
        return;
    }
    const float2 pt = reinterpret_cast<const float2*>(q.points)[vp];
    float2 h = make_float2(0.f, 0.f);
    if (q.headings) h = reinterpret_cast<const float2*>(q.headings)[vp];
    ViewPoint v;
    const bool live = view_point(pt.x, pt.y, q.headings != nullptr, h.x, h.y, v);
    ViewWindow w{0, 0, 0, 0};
    if (live) w = view_window(v, q.R, a.cell, geom.x, geom.y, nx, ny);
    const int wrows = __builtin_amdgcn_readfirstlane(w.i1 - w.i0), wcols = __builtin_amdgcn_readfirstlane(w.j1 - w.j0);
    const int i0 = __builtin_amdgcn_readfirstlane(w.i0), j0 = __builtin_amdgcn_readfirstlane(w.j0);
    const int window = wrows > 0 && wcols > 0 ? wrows*wcols : 0;       // (at most nx*ny <= 2^30)
    const int s = view_slot(q, vp, p);
    const unsigned char* const seen = s >= 0 ? q.unseen + (long long)q.n_maps*a.starts[e] + (long long)s*cells : nullptr;
    const unsigned char* const counts = q.countable + a.starts[e];
    unsigned char* const out = q.values ? q.values + (long long)q.n_points*a.starts[e] + (long long)p*cells : nullptr;

    // the bytes outside the window
    if (out)
        for (int k = tid; k < (int)cells; k += WG) {                    // (an env has at most 2^30 cells: ms_nav_views checks)
            const int i = k / nx, j = k - i*nx;
            if (!((i >= i0) & (i < i0 + wrows) & (j >= j0) & (j < j0 + wcols)) || window == 0) out[k] = 0;
        }

    // the walls that can matter, compacted into LDS in their own order
    const int AF = sc.n_agents*sc.n_model;
    const int L = sc.lines_widths[e];
    const float4* const rows = reinterpret_cast<const float4*>(sc.lines_vals) + sc.lines_starts[e];
    int kept = 0;                                                       // (uniform)
    if (window > 0) {
        const ViewBox box = view_box(v, q.R, a.cell);
        for (int l0 = AF; l0 < L; l0 += WG) {
            const int l = l0 + tid;
            float4 row = make_float4(0.f, 0.f, 0.f, 0.f);
            bool keep = false;
            if (l < L) { row = rows[l]; keep = view_keeps(box, row); }
            const unsigned long long votes = __ballot(keep);
            if (lane == 0) s_kept[wave] = (int)__popcll(votes);
            __syncthreads();
            int at = kept, all = 0;
            for (int k = 0; k < WAVES; k++) { const int c = s_kept[k]; at += k < wave ? c : 0; all += c; }
            at += (int)__popcll(votes & ((1ull << lane) - 1ull));
            if (keep && at < q.capacity) s_walls[at] = row;
            kept += all;
            __syncthreads();
        }
    }
    const bool overflow = kept > q.capacity;                            // (uniform)

    // the cells of the window: a wave a tile of 8 x 8, a lane a cell
    int count = 0, gain = 0;                                            // (uniform within the wave)
    const int tcols = (wcols + VIEW_TILE - 1)/VIEW_TILE, trows = (wrows + VIEW_TILE - 1)/VIEW_TILE;
    const int tiles = window > 0 ? trows*tcols : 0;
    for (int t = wave; t < tiles; t += WAVES) {
        const int ti = t / tcols, tj = t - ti*tcols;
        const int ia = i0 + ti*VIEW_TILE, ja = j0 + tj*VIEW_TILE;        // the tile's first row and column, and its last
        const int ib = min(ia + VIEW_TILE - 1, i0 + wrows - 1), jb = min(ja + VIEW_TILE - 1, j0 + wcols - 1);
        const bool mine = (ia + (lane >> 3) <= ib) & (ja + (lane & 7) <= jb);
        const int i = mine ? ia + (lane >> 3) : ia, j = mine ? ja + (lane & 7) : ja;
        const long long cell = (long long)i*nx + j;
        const float x = nav_centre(geom.x, j, a.cell), y = nav_centre(geom.y, i, a.cell);
        const ViewBox tile = view_tile_box(v, nav_centre(geom.x, ja, a.cell), nav_centre(geom.y, ia, a.cell), nav_centre(geom.x, jb, a.cell),
                                           nav_centre(geom.y, ib, a.cell));
        float rx, ry;
        const bool candidate = mine && view_candidate(v, x, y, q.R2, q.cos_half, rx, ry);
        bool blocked = !candidate;
        if (!overflow) {
            for (int l = 0; l < kept; l++) {
                if (__ballot(!blocked) == 0ull) break;
                const float4 row = s_walls[l];
                if (__ballot(view_keeps(tile, row)) == 0ull) continue;  // (uniform: the wall fails `meets` for every cell of the tile)
                if (!blocked) blocked = view_wall_blocks(v.px, v.py, x, y, rx, ry, row);
            }
        } else {
            for (int l = AF; l < L; l++) {
                if (__ballot(!blocked) == 0ull) break;
                const float4 row = rows[l];
                if (__ballot(view_keeps(tile, row)) == 0ull) continue;
                if (!blocked) blocked = view_wall_blocks(v.px, v.py, x, y, rx, ry, row);
            }
        }
        const bool visible = candidate & !blocked;
        if (out && mine) out[cell] = visible ? 1 : 0;
        const bool counted = visible && (counts[cell] & 1);
        count += (int)__popcll(__ballot(counted));
        if (seen) gain += (int)__popcll(__ballot(counted && !(seen[cell] & 1)));
    }
    if (lane == 0) { s_count[wave] = count; s_gain[wave] = gain; }
    __syncthreads();
    if (tid == 0) {
        int all = 0, fresh = 0;
        for (int k = 0; k < WAVES; k++) { all += s_count[k]; fresh += s_gain[k]; }
        if (q.counts) q.counts[vp] = all;
        if (q.gains) q.gains[vp] = fresh;
    }
}
