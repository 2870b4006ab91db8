// kernels/culltest.h -- the device builds of the culls and shortcuts, element by element, for the test suite (ms_test_*).
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, after the product kernels
// whose functions it calls); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// Where the host and the device compile different text - v_rcp_f32 for a division in wall_beyond, ray_interval,
// pseudo_angle_fast and wg_cell_at; one refined reciprocal for two divisions in tex_filter; light_blocked's sign tests for two
// quotients - a host instantiation says nothing about the device's arithmetic.  These kernels evaluate the very functions the
// product kernels call, one element a lane, on operands a test hands them (tests/test_gpu_culls.py aims them at the
// thresholds).  No LDS, no atomics; they read and write only the `count` elements they are given, any output may be NULL.
// ------------------------------------------------------------------------------------------------

#define MS_TEST_ELEMENT const long long i = (long long)blockIdx.x*WG + threadIdx.x; if (i >= count) return;

__global__ __launch_bounds__(WG) void agents_apart_test_kernel(const float* __restrict__ me, const float* __restrict__ other, const float* __restrict__ radius,
                                                               unsigned char* __restrict__ apart, const long long count) {
    MS_TEST_ELEMENT
    const bool verdict = agents_apart(make_float4(me[4*i], me[4*i + 1], me[4*i + 2], me[4*i + 3]),
                                      make_float4(other[4*i], other[4*i + 1], other[4*i + 2], other[4*i + 3]), radius[i]);
    if (apart) apart[i] = verdict ? 1 : 0;
}

// (as physics_kernel puts them together: the reach from the agent's own row, squared once, every wall against that)
__global__ __launch_bounds__(WG) void wall_beyond_test_kernel(const float* __restrict__ agent, const float* __restrict__ wall, const float* __restrict__ radius,
                                                              float* __restrict__ reach, unsigned char* __restrict__ beyond, const long long count) {
    MS_TEST_ELEMENT
    const float4 tk = make_float4(agent[4*i], agent[4*i + 1], agent[4*i + 2], agent[4*i + 3]);
    const float rch = wall_reach(p2(tk.x, tk.y), p2(tk.z, tk.w), radius[i]);
    const bool verdict = wall_beyond(tk, make_float4(wall[4*i], wall[4*i + 1], wall[4*i + 2], wall[4*i + 3]), reach_squared(rch));
    if (reach) reach[i] = rch;
    if (beyond) beyond[i] = verdict ? 1 : 0;
}

// What ray_interval takes besides the line: the launch's culling constants and the wave's run of rays (ray_span_of, on the host,
// forms them for this kernel and for ms_host_ray_interval_wide alike).
struct RaySpan { float x_clip, c_a, c_b, g0, last_local, n_rays; };
__host__ __device__ inline void ray_interval_of(const float* pose, const float* line, const RaySpan& sp, int& first, int& n) {
    float xa, ya, xb, yb;
    agent_frame(pose[3], pose[2], line[0] - pose[0], line[1] - pose[1], line[2] - pose[0], line[3] - pose[1], xa, ya, xb, yb);
    ray_interval(xa, ya, xb, yb, true, sp.x_clip, sp.c_a, sp.c_b, sp.g0, sp.last_local, first, n, sp.n_rays);
}
__global__ __launch_bounds__(WG) void ray_interval_test_kernel(const float* __restrict__ pose, const float* __restrict__ line, const RaySpan sp,
                                                               int* __restrict__ first, int* __restrict__ rays, const long long count) {
    MS_TEST_ELEMENT
    int lo, n;
    ray_interval_of(pose + 4*i, line + 4*i, sp, lo, n);
    if (first) first[i] = lo;
    if (rays) rays[i] = n;
}

__global__ __launch_bounds__(WG) void wedge_test_kernel(const float* __restrict__ right, const float* __restrict__ left, int* __restrict__ wa, int* __restrict__ wb,
                                                        const long long count) {
    MS_TEST_ELEMENT
    int wa8, wb8;
    wg_wedge(pseudo_angle_fast(right[2*i], right[2*i + 1]), pseudo_angle_fast(left[2*i], left[2*i + 1]), wa8, wb8);
    if (wa) wa[i] = wa8;
    if (wb) wb[i] = wb8;
}

__global__ __launch_bounds__(WG) void cell_at_test_kernel(const float* __restrict__ geom, const float* __restrict__ cell, const float* __restrict__ point,
                                                          int* __restrict__ index, unsigned char* __restrict__ inside, const long long count) {
    MS_TEST_ELEMENT
    bool in;
    const int c = wg_cell_at(make_float4(geom[4*i], geom[4*i + 1], geom[4*i + 2], geom[4*i + 3]), cell[i], point[2*i], point[2*i + 1], in);
    if (index) index[i] = c;
    if (inside) inside[i] = in ? 1 : 0;
}

__global__ __launch_bounds__(WG) void tex_filter_test_kernel(const float* __restrict__ x, const int* __restrict__ w, int* __restrict__ l, int* __restrict__ r,
                                                             float* __restrict__ lw, float* __restrict__ rw, const long long count) {
    MS_TEST_ELEMENT
    const Filt f = tex_filter(x[i], w[i]);
    if (l) l[i] = f.l;
    if (r) r[i] = f.r;
    if (lw) lw[i] = f.lw;
    if (rw) rw[i] = f.rw;
}

__global__ __launch_bounds__(WG) void light_blocked_test_kernel(const float* __restrict__ I, const float* __restrict__ U, const float* __restrict__ a,
                                                                const float* __restrict__ v, unsigned char* __restrict__ blocked, const long long count) {
    MS_TEST_ELEMENT
    const bool verdict = light_blocked(p2(I[2*i], I[2*i + 1]), p2(U[2*i], U[2*i + 1]), a[2*i], a[2*i + 1], v[2*i], v[2*i + 1]);
    if (blocked) blocked[i] = verdict ? 1 : 0;
}

#undef MS_TEST_ELEMENT
