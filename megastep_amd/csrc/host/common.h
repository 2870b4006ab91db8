// host/common.h -- what every family's host side shares: the status of a launch, the checks of the structs every entry takes
// (MsScenery, MsAgents, MsConfig), the small rules of a check (alignment, flags, ranges) and the launch helpers; and the entries
// that belong to no family: ms_abi_version, ms_strerror, ms_last_hip_error, ms_device_count (ms_debug_probe in probe builds).
namespace {
int hip_fail(hipError_t e) { g_last_hip_error = (int)e; return MS_EHIP; }
int launch_status() { const hipError_t e = hipGetLastError(); return e == hipSuccess ? MS_OK : hip_fail(e); }   // (after the launches)

// The small rules of an argument check.  A NULL pointer is aligned (optional pointers are checked for presence where they are
// required); a NaN is neither a flag nor positive.
bool aligned(const void* p, const size_t n) { return (uintptr_t)p % n == 0; }
template <size_t N, typename... P> bool all_aligned(const P*... p) { return (aligned(p, N) && ...); }
bool is_flag(const int x) { return x == 0 || x == 1; }
bool positive_finite(const float x) { return x > 0.f && x < INFINITY; }

// The wave slots render_kernel has on the CURRENT device (CUs x 4 SIMDs x the waves per SIMD its registers are held to): what
// sizes a launch's choice of ray groups and its tail.  Looked up once per device (a process may drive several, of different
// sizes: round 4 kept the first caller's); a benign race - every writer stores the same number.
int wave_slots_here() {
    constexpr int MAX_DEVICES = 64;
    static std::atomic<int> slots_of[MAX_DEVICES];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256*4*MS_WAVES;
    if (dev >= 0 && dev < MAX_DEVICES) { const int known = slots_of[dev].load(std::memory_order_relaxed); if (known) return known; }
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    const int slots = cus*4*MS_WAVES_WIDE;                             // (what sizes launches of wide waves: theirs)
    if (dev >= 0 && dev < MAX_DEVICES) slots_of[dev].store(slots, std::memory_order_relaxed);
    return slots;
}

bool scenery_ok(const MsScenery* s) {
    return s && s->n_envs > 0 && s->n_agents > 0 && s->n_model > 0 && s->lines_vals && s->lines_widths &&
           s->lines_starts && s->model && all_aligned<16>(s->lines_vals, s->model);
}
bool agents_ok(const MsAgents* a) { return a && a->angles && a->positions && a->angvelocity && a->velocity; }
bool config_ok(const MsConfig* c) {
    return c && c->res > 0 && c->fps > 0.f && c->agent_radius > 0.f && c->fov > 0.f && c->fov < 180.f;
}
AgentsK agents_or_none(const MsAgents* a) { return a ? agents_k(*a) : AgentsK{nullptr, nullptr, nullptr, nullptr, nullptr}; }
// Agents an entry may go without (ray queries, pictures from above, clearance of points): given, they have poses.
bool posed_or_none_ok(const MsAgents* a) { return !a || (a->angles && a->positions && aligned(a->positions, 8)); }

// kernels.cu:22: the camera's half-width at unit distance, as every launch that casts its rays works it out
float half_screen_of(const float fov) { return tanf(3.14159265358979323846f/180.f*fov/2.); }

// The light grid is all or nothing: render_kernel lights agent-hit rays itself when it is there.
bool light_grid_in(const MsScenery* sc) { return sc->lg_vals && sc->lg_starts && sc->lg_geom && sc->lg_cell > 0.f; }
// The wall grid's vis lists serve rays of this near plane: they were built for near planes below wg_near (wallgrid_scan_kernel).
bool vis_lists_serve(const MsScenery* sc, const float near_plane) {
    return sc->wg_cells && sc->wg_starts && sc->wg_geom && sc->wg_pool && sc->wg_pool_base && sc->wg_cell > 0.f &&
           near_plane*1.001f < sc->wg_near;
}

// One element a lane (arithmetic_test_kernel and kernels/culltest.h): `ok` = every pointer the kernel reads is there.
template <typename... Params, typename... Args>
int launch_elements(void (*kernel)(Params...), const bool ok, const long long count, void* stream, Args... args) {
    if (count < 0 || !ok) return MS_EINVAL;
    if (count == 0) return MS_OK;
    const long long blocks = (count + WG - 1)/WG;
    if (blocks > 0x7fffffffLL) return MS_EUNSUPPORTED;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(WG), 0, (hipStream_t)stream, args..., count);
    return launch_status();
}

// A launch whose dynamic LDS may pass the 64 KiB a kernel gets unasked: beyond `threshold` bytes (the caller's: 64 KiB less the
// kernel's static LDS) the kernel is allowed as much first.  MS_OK, or MS_EHIP with nothing launched.
template <typename... Params>
int allow_dynamic_lds(void (*kernel)(Params...), const size_t bytes, const size_t threshold) {
    if (bytes > threshold && hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)bytes) != hipSuccess) return hip_fail(hipGetLastError());
    return MS_OK;
}
}  // namespace

extern "C" {
int ms_abi_version(void) { return MS_ABI_VERSION; }

const char* ms_strerror(int code) {
    switch (code) {
        case MS_OK: return "ok";
        case MS_EINVAL: return "invalid argument (null/misaligned pointer, non-positive size or bad config)";
        case MS_EHIP: return "a HIP runtime call failed (see ms_last_hip_error)";
        case MS_EUNSUPPORTED: return "shape not supported by the gfx950 kernels";
        case MS_ENODEVICE: return "no HIP device visible";
        default: return "unknown megastep_hip error";
    }
}

int ms_last_hip_error(void) { return g_last_hip_error; }

int ms_device_count(void) {
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { g_last_hip_error = (int)e; return MS_ENODEVICE; }
    return n;
}

#if MS_PROBE
// (probe builds only, not part of the ABI) buf: device memory of capacity records of 11 32-bit words (8 stamps, HW_ID |
// XCC_ID << 16, the real-time counter at the wave's start and end), or NULL to stop recording
int ms_debug_probe(unsigned* buf, long long capacity) {
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_probe), &buf, sizeof buf) != hipSuccess) return hip_fail(hipGetLastError());
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_probe_cap), &capacity, sizeof capacity) != hipSuccess) return hip_fail(hipGetLastError());
    return MS_OK;
}
#endif
}  // extern "C"
