// host.hpp -- the host mechanisms the entries of api.hip and inspect.hip use but do not define (host.hip): the calling thread's error
// text, the check behind every launch, the per-step timing, the landing zone of the counter read-back, and the record of what the
// last forward on a geometry arena saved.  No kernel lives in host.hip.
#pragma once

#include "common.hpp"

namespace gsr {

// stores the message in the calling thread's error buffer (gsr_last_error) and returns `code`
int fail(int code, const char* fmt, ...);
const char* last_error();

int check_launch(const Launch& L, const char* what);

// what the entries of both units read off a call's sizes
inline int tile_count(const gsr_params* p) { return ((p->W + TILE_X - 1) / TILE_X) * ((p->H + TILE_Y - 1) / TILE_Y); }
// how many u32 tile-key bits the tile sort covers: the reference's 32+bit minus the 32 depth bits
inline int tile_bits(int T) { return (int)higher_msb((uint32_t)T); }
// which of the two ping-pong buffers holds the sorted lists (depends on the pass count only)
inline int sorted_buffer(int T) { return ((tile_bits(T) + RADIX_BITS - 1) / RADIX_BITS) & 1; }
inline void* align256(void* p) { return (void*)(((uintptr_t)p + 255) & ~(uintptr_t)255); }

// ---- optional per-step timing (hipEvents on the launch stream) -------------------------------------
// Records are kept PER STREAM (several host threads may render at once, each on its own stream, and one frame's forward
// and backward usually come from different host threads -- autograd runs the backward on its own thread -- but on the
// same stream).  The switch is process wide.
struct ProfScope {
    hipStream_t s;
    bool on;
    const char* name;
    int a, b;  // indices into the stream's event pool
    ProfScope(const char* name, hipStream_t stream);
    ~ProfScope();
    ProfScope(const ProfScope&) = delete;
    ProfScope& operator=(const ProfScope&) = delete;
};
void set_profiling(int on);                                 // gsr_set_profiling: 0 off, 1 every stage, 2 the two render kernels only
int get_profile(const char** names, float* ms, int cap);    // gsr_get_profile

// ---- per-thread landing zone for the counter read-back ----------------------------------------------------
// Host memory mapped into the device: the pair-emission kernel stores the per-view counters there itself, and the host
// reads them after an event recorded behind that kernel.  No copy command (on this runtime a small device->host copy is a
// blit kernel plus two ~10 us bubbles in the stream).
constexpr int MAX_VIEWS = 256;
// One per (host thread, device): an event belongs to the device that was current when it was created, so a thread that
// renders on several GPUs needs one landing zone for each.
struct HostLanding {
    uint64_t* pinned = nullptr;   // [MAX_VIEWS][4]: num_rendered, trap flag, stall flag, -   (host address)
    uint64_t* mapped = nullptr;   // the same memory as the device sees it
    hipEvent_t ev = nullptr;
};
int landing(HostLanding** out);   // the calling thread's, for the current device

// What the last forward on a geometry arena saved for the backward, kept on the host so that gsr_backward_batch and
// gsr_backward_batch_channels can refuse a backward that does not match it without reading anything back from the device.  Keyed by
// the arena's address: every forward and recolor on an arena rewrites its record.
struct FrameRecord {
    int kind = 0;             // 0 colour forward, 1 channels forward, 2 recolor
    int need_backward = 0;
    int nx = 0, layout = 0;   // channels forwards
    int V = 0, P = 0, W = 0, H = 0;
    const void* xstate = nullptr;   // the extra-state block the channels forward saved into (NULL: none)
    size_t xstate_bytes = 0;
    int fwd_need_backward = -1;  // need_backward of the forward whose geometry and lists the arena holds (a recolor carries it on;
                                 // -1: unknown, a recolor on an arena without a record)
    int64_t list_pairs = -1;     // largest per-view pair count of that forward's lists (a recolor carries it on; -1: unknown): what the
                                 // scratch of a deterministic backward has to hold slots for
    int math = 0;                // arithmetic of the call that last wrote the colour saves (0 exact, 1 fast): the forward, or a recolor --
                                 // it rewrites final_T and n_contrib of every pixel and, through the same kernel, every slice-boundary
                                 // state and accumulated colour a backward reads.  The render backward runs the same mode.
    int bwd_done = 0;            // a backward has run since this record was written (every forward and recolor writes a fresh one):
                                 // the gradient records hold its sums, which is what gsr_backward_cameras reads
    FrameRecord() = default;
    FrameRecord(int kind_, const gsr_params* p, int V_) : kind(kind_), need_backward(p->need_backward != 0), V(V_), P(p->P), W(p->W), H(p->H) {}
};
void note_frame(const void* geom, const FrameRecord& r);
bool find_frame(const void* geom, FrameRecord& r);
// read-modify-write of an arena's record under one lock (no record: nothing happens)
void update_frame(const void* geom, void (*change)(FrameRecord&));

// The one check of an arena's record for the entries that run on the arenas of a finished forward or recolor: `who` (the entry's
// name in the messages) needs the last forward / recolor to have saved for a backward (GATE_SAVES; saves_tail ends that message),
// a backward to have run since (GATE_RECORDS), and always the same V, P, W, H -- asked in this order.  Without a record (an arena
// whose forward ran before the record table was last dropped, at more than 4096 arenas) the call goes ahead as it always did:
// refusing it would break a valid call, and the callers' contract (gsr.h) is unchanged.  Returns through `out` (may be NULL) the
// record, and through `known` whether there is one.
enum { GATE_SAVES = 1, GATE_RECORDS = 2 };
int frame_gate(const char* who, const void* geom, const gsr_params* p, int V, int needs, const char* saves_tail,
               FrameRecord* out = nullptr, bool* known = nullptr);

}  // namespace gsr
