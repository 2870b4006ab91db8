// kernels/shade.h -- shade_kernel, camera_pose_rays_kernel, shade_serial (ms_host_shade).
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, after raycast.h: it uses
// render.h's texel filter, draw and camera-ray helpers and lighting.h's shadow test and light grid); not a header to compile
// on its own.
// ------------------------------------------------------------------------------------------------
// shading of rays the caller gives: the reference's shader_kernel                  kernels.cu:407-450
// ------------------------------------------------------------------------------------------------
// The render shades the rays it casts itself.  ms_shade applies the same rule to the planes ms_raycast wrote
// for ANY rays - a rear view, a panorama, a fixed camera - one ray per lane, rays of one env next to each other (raycast_kernel's
// indexing: ray i = n R + r).  Nothing is written but `screen`: an agent's row is drawn in registers from its live pose.
//
// The per-ray steps are functions of their own, shared by the kernel and by shade_serial, the serial host statement behind
// ms_host_shade.  On the device each is the render's own operation (tex_filter, drawn_row, light_blocked); on the host, which
// has no v_rcp_f32, the same correctly rounded quotients come from plain divisions (math.h, div_inrange: in range the refined
// sequence IS the correctly rounded quotient).

// kernels.cu:394-405: the two texels under a hit and their weights
__host__ __device__ inline Filt shade_filter(const float x, const int w) {
#if defined(__HIP_DEVICE_COMPILE__)
    return tex_filter(x, w);
#else
    Filt f;
    const float y = ms_min(x*(w + 1), (float)(w - 1));
    f.l = (int)ms_max(y - 1, 0.f);
    f.r = (int)ms_min(y, (float)(w - 1));
    const float ld = fabsf(y - (f.l + 1)) + 1.e-3f;
    const float rd = fabsf(y - (f.r + 1)) + 1.e-3f;
    const float den = ld + rd;
    f.lw = rd/den;
    f.rw = ld/den;
    return f;
#endif
}
// kernels.cu:305-314: a model row at a pose
__host__ __device__ inline float4 shade_row(const float s, const float c, const float px, const float py, const float4 mdl) {
#if defined(__HIP_DEVICE_COMPILE__)
    return drawn_row(s, c, px, py, mdl);
#else
    float4 w;
    w.x = c*mdl.x - s*mdl.y + px; w.y = s*mdl.x + c*mdl.y + py;
    w.z = c*mdl.z - s*mdl.w + px; w.w = s*mdl.z + c*mdl.w + py;
    return w;
#endif
}
// kernels.cu:238-259 `obstructed`: does the wall (a, a + v) stand between the light I and the point I + U?
__host__ __device__ inline bool shade_blocked(const P2 I, const P2 U, const float ax, const float ay, const float vx, const float vy) {
#if defined(__HIP_DEVICE_COMPILE__)
    return light_blocked(I, U, ax, ay, vx, vy);
#else
    const P2 V = p2(vx, vy);
    const float UxV = cross(U, V);
    if (fabsf(UxV) < 1.e-3f) return false;
    const P2 PQ = p2(ax, ay) - I;
    const float t = cross(PQ, U)/UxV, s = cross(PQ, V)/UxV;
    return (t > 0.f) & (t < 1.f) & (s > 0.f) & (s < .999f);
#endif
}

// What a ray's index says, against its env's L lines of which the first AF are the agents': nothing to shade (a miss, or an
// index that is no line of the env - nothing is read for it), an agent's row, a static line.
enum ShadeKind { SHADE_BLACK = 0, SHADE_AGENT = 1, SHADE_STATIC = 2 };
__host__ __device__ inline int shade_kind(const int idx, const int L, const int AF) {
    if ((idx < 0) | (idx >= L)) return SHADE_BLACK;
    return idx < AF ? SHADE_AGENT : SHADE_STATIC;
}
// A location is a place along a line: ms_raycast writes nothing else for a hit.  Any other bit pattern a caller hands over - a NaN,
// an infinity, 2 - has no texel under it (and (int) of it is anything): such a ray is black too.
__host__ __device__ inline bool shade_on_line(const float loc) { return (loc >= 0.f) & (loc <= 1.f); }
// The hit point on agent row `idx` of env n (kernels.cu:435), the row drawn from the agent's pose as it is now.
__host__ __device__ inline P2 shade_agent_point(const float* angles, const float* positions, const float* model, const int A, const int M,
                                                const int n, const int idx, const float loc) {
    const int a = idx / M, m = idx - a*M;
    float s, c;
    sincospi_f(angles[n*A + a]/180.f, s, c);
    const float px = positions[2*(n*A + a)], py = positions[2*(n*A + a) + 1];
    const float4 hw = shade_row(s, c, px, py, reinterpret_cast<const float4*>(model)[m]);
    return p2(hw.x*(1 - loc) + hw.z*loc, hw.y*(1 - loc) + hw.w*loc);
}
// kernels.cu:261-264: an unblocked light's share, added to the running sum
__host__ __device__ inline float shade_lit(const float acc, const P2 I, const float Ii, const P2 C) {
    const float d2 = len2(I - C);
    return acc + LUMINANCE*Ii/ms_max(d2, 1.f);
}
// A texel index kept inside its row: what tex_filter gives it is, for a location in [0, 1] - the clamp changes nothing, and no
// index computed from a caller's floats is used as an address unchecked.
__host__ __device__ inline int shade_texel(const int t, const int w) { return t < 0 ? 0 : (t > w - 1 ? w - 1 : t); }
// kernels.cu:437-445: intensity on a static line, and the triple
__host__ __device__ inline float shade_baked(const float* baked, const int tstart, const Filt f, const int w) {
    return f.lw*baked[tstart + shade_texel(f.l, w)] + f.rw*baked[tstart + shade_texel(f.r, w)];
}
__host__ __device__ inline void shade_colour(const float* tex, const int tstart, const Filt f, const int w, const float intensity, const float dt,
                                             float& s0, float& s1, float& s2) {
    const float* const tl = tex + 3*(size_t)(tstart + shade_texel(f.l, w));
    const float* const tr = tex + 3*(size_t)(tstart + shade_texel(f.r, w));
    const float dn = 1 - dt*dt;
    s0 = dn*intensity*(f.lw*tl[0] + f.rw*tr[0]);
    s1 = dn*intensity*(f.lw*tl[1] + f.rw*tr[1]);
    s2 = dn*intensity*(f.lw*tl[2] + f.rw*tr[2]);
}

// Ray i = n R + r of the launch.  with_agents: the caller gave the agents' poses - else a ray on an agent's row leaves black.
// gridded: the scenery's light grid serves (the host checked it): the agent hits of a wave go through grid_light_intensity, env
// segment by env segment (it takes a wave-uniform env; a wave holds two envs' rays when R is no multiple of 64).  Without a grid
// - single-agent sceneries have none, and a free camera still sees their agent - the wave takes its agent-hit rays one after the
// other, in lane order, and each one's lights in the lights' order: the lanes share out the env's static rows, a ballot says
// whether any of them blocks the light, and the sum is the reference's, term by term.
__global__ __launch_bounds__(WG) void shade_kernel(const MsScenery sc, const AgentsK ag, const MsShade q, const int with_agents,
                                                   const int gridded, const Divisor by_m, const int n_total) {
    __shared__ LightPair s_pair[WAVES][LG_PAIRS];
    __shared__ unsigned s_shadow[WAVES][2*WAVE];
    const int lane = (int)threadIdx.x % WAVE, wave = (int)threadIdx.x / WAVE;
    const int i_raw = blockIdx.x*WG + threadIdx.x;
    const bool live = i_raw < n_total;
    const int i = live ? i_raw : n_total - 1;                           // (spare lanes of the last block redo its last ray, store nothing)
    const int n = i / q.n_rays;
    const int A = sc.n_agents, M = sc.n_model, AF = A*M;
    const int idx = q.indices[i];
    const float loc = q.locations[i], dt = q.dots[i];
    const int L = sc.lines_widths[n], base = sc.lines_starts[n];
    const int kind = shade_kind(idx, L, AF);
    const bool dynamic = (kind == SHADE_AGENT) & (with_agents != 0);
    const bool is_hit = dynamic | (kind == SHADE_STATIC);
    // the winner's texel row and the filter under the hit: a handful of gathers, for the lanes that have something to shade
    int tex_w = 0, tstart = 0;
    if (is_hit) { tex_w = sc.textures_widths[base + idx]; tstart = sc.textures_starts[base + idx]; }
    const bool shaded = is_hit & (tex_w >= 1) & shade_on_line(loc);
    Filt f = Filt{0, 0, 0.f, 0.f};
    float intensity = 0.f;
    if (shaded) {
        f = shade_filter(loc, tex_w);
        if (!dynamic) intensity = shade_baked(sc.baked_vals, tstart, f, tex_w);
    }
    // ---- rays on an agent's body: light_intensity at the hit point (kernels.cu:432-436)
    const bool lit = shaded & dynamic;
    if (__ballot(lit)) {
        P2 C = p2(0.f, 0.f);
        if (lit) C = shade_agent_point(ag.angles, ag.positions, sc.model, A, M, n, idx, loc);
        if (gridded) {
            const LightScene scl{sc.n_agents, sc.n_model, sc.lights_vals, sc.lights_widths, sc.lights_starts, sc.lg_vals, sc.lg_starts,
                                 sc.lg_geom, sc.lg_cell, sc.lg_list, sc.lg_pool, reinterpret_cast<const float4*>(sc.lg_pool_rows),
                                 by_m.mul, by_m.sh1, by_m.sh2};
            for (unsigned long long todo = __ballot(lit); todo;) {       // (uniform: every lane walks every segment)
                const int n_s = __builtin_amdgcn_readlane(n, __ffsll((long long)todo) - 1);
                const bool mine = lit & (n == n_s);
                todo &= ~__ballot(mine);
                const int L_s = sc.lines_widths[n_s];
                const float4* const ln = reinterpret_cast<const float4*>(sc.lines_vals) + sc.lines_starts[n_s];
                unsigned telemetry = 0u;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const float v = grid_light_intensity(scl, ag, n_s, lane, mine, idx, C.x, C.y, L_s, ln, s_pair[wave], s_shadow[wave], telemetry);
                if (mine) intensity = v;
            }
        } else {
            for (unsigned long long todo = __ballot(lit); todo; todo &= todo - 1) {
                const int j = __ffsll((long long)todo) - 1;
                const int n_j = __builtin_amdgcn_readlane(n, j);
                const P2 Cj = p2(readlane_f(C.x, j), readlane_f(C.y, j));
                const int L_j = sc.lines_widths[n_j], n_lights = sc.lights_widths[n_j];
                const float4* const rows = reinterpret_cast<const float4*>(sc.lines_vals) + sc.lines_starts[n_j];
                const float* const lights = sc.lights_vals + 3*(size_t)sc.lights_starts[n_j];
                float acc = AMBIENT;
                for (int k = 0; k < n_lights; k++) {
                    const P2 I = p2(lights[3*k], lights[3*k + 1]);
                    const float Ii = lights[3*k + 2];
                    const P2 U = Cj - I;
                    bool blocked = false;
                    for (int l0 = AF; l0 < L_j && !blocked; l0 += WAVE) {       // (only the static rows block)
                        bool mine = false;
                        if (l0 + lane < L_j) {
                            const float4 w = rows[l0 + lane];
                            mine = shade_blocked(I, U, w.x, w.y, w.z - w.x, w.w - w.y);
                        }
                        blocked = __ballot(mine) != 0ull;
                    }
                    if (!blocked) acc = shade_lit(acc, I, Ii, Cj);
                }
                if (lane == j) intensity = ms_min(acc, 1.f);
            }
        }
    }
    if (!live) return;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    if (shaded) shade_colour(sc.textures_vals, tstart, f, tex_w, intensity, dt, s0, s1, s2);
    q.screen[3*(size_t)i] = s0; q.screen[3*(size_t)i + 1] = s1; q.screen[3*(size_t)i + 2] = s2;
}

// The serial host statement of the same rule, on host arrays: ray after ray, each step the function the kernel calls, the
// lights taken the plain way - light after light, row after row.
inline void shade_serial(const MsScenery& sc, const MsAgents* ag, const MsShade& q) {
    const int A = sc.n_agents, M = sc.n_model, AF = A*M;
    for (int n = 0; n < sc.n_envs; n++) {
        const int L = sc.lines_widths[n], base = sc.lines_starts[n];
        const float4* const rows = reinterpret_cast<const float4*>(sc.lines_vals) + base;
        const int n_lights = sc.lights_widths[n];
        const float* const lights = n_lights > 0 ? sc.lights_vals + 3*(size_t)sc.lights_starts[n] : nullptr;
        for (int r = 0; r < q.n_rays; r++) {
            const size_t i = (size_t)n*q.n_rays + r;
            const int idx = q.indices[i];
            const float loc = q.locations[i], dt = q.dots[i];
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
            const int kind = shade_kind(idx, L, AF);
            const bool dynamic = kind == SHADE_AGENT && ag;
            if (dynamic || kind == SHADE_STATIC) {
                const int tex_w = sc.textures_widths[base + idx], tstart = sc.textures_starts[base + idx];
                if (tex_w >= 1 && shade_on_line(loc)) {
                    const Filt f = shade_filter(loc, tex_w);
                    float intensity;
                    if (dynamic) {
                        const P2 C = shade_agent_point(ag->angles, ag->positions, sc.model, A, M, n, idx, loc);
                        float acc = AMBIENT;
                        for (int k = 0; k < n_lights; k++) {
                            const P2 I = p2(lights[3*k], lights[3*k + 1]);
                            const P2 U = C - I;
                            bool blocked = false;
                            for (int l = AF; l < L && !blocked; l++)
                                blocked = shade_blocked(I, U, rows[l].x, rows[l].y, rows[l].z - rows[l].x, rows[l].w - rows[l].y);
                            if (!blocked) acc = shade_lit(acc, I, lights[3*k + 2], C);
                        }
                        intensity = ms_min(acc, 1.f);
                    } else {
                        intensity = shade_baked(sc.baked_vals, tstart, f, tex_w);
                    }
                    shade_colour(sc.textures_vals, tstart, f, tex_w, intensity, dt, s0, s1, s2);
                }
            }
            q.screen[3*i] = s0; q.screen[3*i + 1] = s1; q.screen[3*i + 2] = s2;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// rays of free cameras
// ------------------------------------------------------------------------------------------------
// Camera c of env n stands at pose (x, y, heading in degrees) and casts `res` rays, ray 0 leftmost as in the render: ray
// k = c res + r of the env's C res.  MS_CAMERA_PLANE: the render's projection - the heading through sincospi_f(heading/180)
// and the column's ray by camera_ray, exactly as camera_rays_kernel forms them (direction vectors of length 1 .. sqrt(1 +
// half_screen^2)).  MS_CAMERA_RING: the rays fan out evenly in angle - ray r points along heading + fov (res - 2r - 1)/(2 res)
// degrees, through sincospi_f: unit vectors, any fov up to the whole turn.
__global__ __launch_bounds__(WG) void camera_pose_rays_kernel(const MsCameraPoses q, const float half_screen, const float inv_res, const long long total) {
    const long long i = (long long)blockIdx.x*WG + threadIdx.x;
    if (i >= total) return;
    const long long cam = i / q.res;
    const int r = (int)(i - cam*q.res);
    const float x = q.poses[3*cam], y = q.poses[3*cam + 1], heading = q.poses[3*cam + 2];
    float s, c, rx, ry;
    if (q.projection == MS_CAMERA_RING) {
        const float turn = q.fov*(float)(q.res - 2*r - 1)/(float)(2*q.res);
        sincospi_f((heading + turn)/180.f, s, c);
        rx = c; ry = s;
    } else {
        sincospi_f(heading/180.f, s, c);
        camera_ray(c, s, r, (float)q.res, half_screen, inv_res, rx, ry);
    }
    reinterpret_cast<float2*>(q.origins)[i] = make_float2(x, y);
    reinterpret_cast<float2*>(q.dirs)[i] = make_float2(rx, ry);
}
