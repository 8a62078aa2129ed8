// host.hip -- the host state behind host.hpp.  Host code only: this unit holds no kernel.
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "host.hpp"

namespace gsr {

static thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

const char* last_error() { return g_err; }

int check_launch(const Launch& L, const char* what)
{
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && L.debug) e = hipStreamSynchronize(L.stream);  // CHECK_CUDA(…, debug) of the reference
    if (e != hipSuccess) return fail(GSR_ERR_HIP, "[gsr] %s: %s", what, hipGetErrorString(e));
    return GSR_OK;
}

// ---- per-step timing ----
struct ProfEntry {
    const char* name;
    int a, b;
};
struct ProfTables {
    std::vector<hipEvent_t> pool;
    size_t used = 0;
    std::vector<ProfEntry> rec;
    int event()
    {
        if (used == pool.size()) {
            // timing events only: no system-scope fence when they are recorded (hipEventRecord's default release writes the L2s back
            // and invalidates them between two stages, so the kernel behind an event pair started cold: the per-stage pass read
            // k_render_backward 7-10 % slower than the kernel trace of the same run, profiles/r04_bench_kernel_stats.csv)
            hipEvent_t e;
            if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) (void)hipEventCreate(&e);
            pool.push_back(e);
        }
        return (int)used++;
    }
};
static std::atomic<int> g_prof_on{0};    // 0 off, 1 every stage, 2 the two render kernels only (cheap enough for a timed region)
static std::mutex g_prof_mu;
static std::map<hipStream_t, ProfTables> g_prof;   // guarded by g_prof_mu

ProfScope::ProfScope(const char* name_, hipStream_t stream) : s(stream), on(false), name(name_), a(0), b(0)
{
    const int mode = g_prof_on;
    on = mode == 1 || (mode == 2 && strncmp(name, "render_", 7) == 0);
    if (!on) return;
    hipEvent_t ea;
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        ProfTables& t = g_prof[s];
        a = t.event();
        b = t.event();
        ea = t.pool[a];
    }
    (void)hipEventRecord(ea, s);
}

ProfScope::~ProfScope()
{
    if (!on) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    ProfTables& t = g_prof[s];
    (void)hipEventRecord(t.pool[b], s);
    t.rec.push_back(ProfEntry{name, a, b});
}

void set_profiling(int on)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_on = on < 0 ? 0 : on > 2 ? 1 : on;
    for (auto& kv : g_prof) { kv.second.rec.clear(); kv.second.used = 0; }
}

int get_profile(const char** names, float* ms, int cap)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    int n = 0;
    for (auto& kv : g_prof) {
        ProfTables& t = kv.second;
        for (auto& e : t.rec) {
            if (n >= cap) break;
            (void)hipEventSynchronize(t.pool[e.b]);
            float d = 0;
            (void)hipEventElapsedTime(&d, t.pool[e.a], t.pool[e.b]);
            names[n] = e.name;
            ms[n] = d;
            n++;
        }
        t.rec.clear();
        t.used = 0;
    }
    return n;
}

// ---- landing zone ----
static thread_local std::map<int, HostLanding> t_lands;
int landing(HostLanding** out)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(GSR_ERR_HIP, "[gsr] hipGetDevice: %s", hipGetErrorString(hipGetLastError()));
    HostLanding& h = t_lands[dev];
    if (!h.pinned) {
        if (hipHostMalloc((void**)&h.pinned, MAX_VIEWS * 4 * sizeof(uint64_t), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
            hipHostGetDevicePointer((void**)&h.mapped, h.pinned, 0) != hipSuccess ||
            // (hipEventDisableSystemFence on this event was tried -- the counters live in coherent host memory and the kernel fences
            // them itself, so the record would not need the system-scope release of the L2s -- and cost the per-view path a fifth of
            // its rate, 1 363 -> 1 050-1 130 frames/s, gpurun_out/r4m: waiting for such an event does not return when the emission
            // kernel ends but when the stream drains, and the host stops running ahead of the device)
            hipEventCreateWithFlags(&h.ev, hipEventDisableTiming) != hipSuccess) {
            h.pinned = nullptr;
            return fail(GSR_ERR_HIP, "[gsr] pinned host buffer: %s", hipGetErrorString(hipGetLastError()));
        }
    }
    *out = &h;
    return GSR_OK;
}

// ---- frame records ----
static std::mutex g_frames_mu;
static std::map<const void*, FrameRecord> g_frames;
void note_frame(const void* geom, const FrameRecord& r)
{
    std::lock_guard<std::mutex> lk(g_frames_mu);
    if (g_frames.size() > 4096 && !g_frames.count(geom)) g_frames.clear();   // (arenas come and go; records of freed ones are dropped)
    g_frames[geom] = r;
}
bool find_frame(const void* geom, FrameRecord& r)
{
    std::lock_guard<std::mutex> lk(g_frames_mu);
    const auto it = g_frames.find(geom);
    if (it == g_frames.end()) return false;
    r = it->second;
    return true;
}
void update_frame(const void* geom, void (*change)(FrameRecord&))
{
    std::lock_guard<std::mutex> lk(g_frames_mu);
    const auto it = g_frames.find(geom);
    if (it != g_frames.end()) change(it->second);
}

int frame_gate(const char* who, const void* geom, const gsr_params* p, int V, int needs, const char* saves_tail, FrameRecord* out,
               bool* known)
{
    FrameRecord r;
    const bool found = find_frame(geom, r);
    if (out) *out = r;
    if (known) *known = found;
    if (!found) return GSR_OK;
    if ((needs & GATE_SAVES) && !r.need_backward)
        return fail(GSR_ERR_INVALID, "[gsr] %s: the last %s on this geometry arena had need_backward = 0%s", who,
                    r.kind == 2 ? "gsr_forward_recolor" : "forward", saves_tail);
    if ((needs & GATE_RECORDS) && !r.bwd_done)
        return fail(GSR_ERR_INVALID, "[gsr] %s: no backward has run since the last forward or recolor on this geometry arena (the "
                    "gradient records are empty; run one of the gsr_backward entries first)", who);
    if (r.V != V || r.P != p->P || r.W != p->W || r.H != p->H)
        return fail(GSR_ERR_INVALID, "[gsr] %s: V = %d, P = %d, %d x %d, but the last forward or recolor on this geometry arena "
                    "had V = %d, P = %d, %d x %d", who, V, p->P, p->W, p->H, r.V, r.P, r.W, r.H);
    return GSR_OK;
}

}  // namespace gsr
