// host/probes.h -- the ms_test_* probes (kernels/culltest.h and math.h's arithmetic_test_kernel: the device builds of the culls
// and shortcuts, an element a lane) and the host hooks of the same predicates: ms_host_ray_interval*, ms_host_agents_apart,
// ms_host_wall_reach, ms_host_wall_beyond_reach, ms_host_sincospi.
namespace {
// ray_interval's launch-invariant values as ms_render works them out, the per-wave ones as render_kernel does: wave `wave` of
// 64 x groups rays (ms_host_ray_interval_wide and ms_test_ray_interval)
RaySpan ray_span_of(const int res, const float fov, const float agent_radius, const int groups, const int wave) {
    const float half_screen = half_screen_of(fov);
    const float x_clip = 0.5f*agent_radius/sqrtf(1.f + half_screen*half_screen), c_b = 0.5f*(float)res/half_screen;
    const int nr = WAVE*groups, r0 = wave*nr;
    const float c_a = 0.5f*((float)res - 1.f), g0 = (float)r0;
    const int r_last = (r0 + nr - 1 < res - 1) ? r0 + nr - 1 : res - 1;
    return RaySpan{x_clip, c_a, c_b, g0, (float)(r_last - r0), (float)nr};
}
}  // namespace

extern "C" {
void ms_host_sincospi(float x, float* s, float* c) { sincospi_f(x, *s, *c); }

int ms_test_arithmetic(const float* n, const float* d, float* q_inrange, float* q_ieee, const float* x, float* r_any, float* r_ieee,
                       long long count, void* stream) {
    const bool ok = !((q_inrange || q_ieee) && !(n && d)) && !((r_any || r_ieee) && !x);
    return launch_elements(arithmetic_test_kernel, ok, count, stream, n, d, q_inrange, q_ieee, x, r_any, r_ieee);
}
int ms_test_agents_apart(const float* me, const float* other, const float* radius, unsigned char* apart, long long count, void* stream) {
    return launch_elements(agents_apart_test_kernel, me && other && radius, count, stream, me, other, radius, apart);
}
int ms_test_wall_beyond(const float* agent, const float* wall, const float* radius, float* reach, unsigned char* beyond, long long count,
                        void* stream) {
    return launch_elements(wall_beyond_test_kernel, agent && wall && radius, count, stream, agent, wall, radius, reach, beyond);
}
int ms_test_ray_interval(const float* pose, const float* line, int res, float fov, float agent_radius, int groups, int wave, int* first,
                         int* rays, long long count, void* stream) {
    // (a wave of a launch ms_render could make: config_ok's ranges, NG of 1, 2 or 4, a run of rays that starts below res)
    if (!(res > 0 && fov > 0.f && fov < 180.f && agent_radius > 0.f && (groups == 1 || groups == 2 || groups == 4) && wave >= 0 &&
          (long long)wave*WAVE*groups < res)) return MS_EINVAL;
    return launch_elements(ray_interval_test_kernel, pose && line, count, stream, pose, line, ray_span_of(res, fov, agent_radius, groups, wave), first, rays);
}
int ms_test_wedge(const float* right, const float* left, int* wa, int* wb, long long count, void* stream) {
    return launch_elements(wedge_test_kernel, right && left, count, stream, right, left, wa, wb);
}
int ms_test_cell_at(const float* geom, const float* cell, const float* point, int* index, unsigned char* inside, long long count, void* stream) {
    return launch_elements(cell_at_test_kernel, geom && cell && point, count, stream, geom, cell, point, index, inside);
}
int ms_test_tex_filter(const float* x, const int* w, int* l, int* r, float* lw, float* rw, long long count, void* stream) {
    return launch_elements(tex_filter_test_kernel, x && w, count, stream, x, w, l, r, lw, rw);
}
int ms_test_light_blocked(const float* light, const float* to, const float* a, const float* v, unsigned char* blocked, long long count,
                          void* stream) {
    return launch_elements(light_blocked_test_kernel, light && to && a && v, count, stream, light, to, a, v, blocked);
}

void ms_host_ray_interval_wide(const float* pose, const float* line, int res, float fov, float agent_radius, int groups, int wave,
                               int* first, int* count) {
    ray_interval_of(pose, line, ray_span_of(res, fov, agent_radius, groups, wave), *first, *count);
}
void ms_host_ray_interval(const float* pose, const float* line, int res, float fov, float agent_radius, int group, int* first, int* count) {
    ms_host_ray_interval_wide(pose, line, res, fov, agent_radius, 1, group, first, count);
}

float ms_host_wall_reach(const float* agent, float agent_radius) { return wall_reach(p2(agent[0], agent[1]), p2(agent[2], agent[3]), agent_radius); }

int ms_host_wall_beyond_reach(const float* agent, const float* wall, float agent_radius) {
    const float reach = wall_reach(p2(agent[0], agent[1]), p2(agent[2], agent[3]), agent_radius);
    return wall_beyond(make_float4(agent[0], agent[1], agent[2], agent[3]), make_float4(wall[0], wall[1], wall[2], wall[3]),
                       reach_squared(reach)) ? 1 : 0;
}

int ms_host_agents_apart(const float* me, const float* other, float agent_radius) {
    return agents_apart(make_float4(me[0], me[1], me[2], me[3]), make_float4(other[0], other[1], other[2], other[3]), agent_radius) ? 1 : 0;
}
}  // extern "C"
