// Phase stamps of the fused-clear tile kernel (splat_body), for the diagnostic build -DACCV_SPLAT_STAMPS only
// (scripts/splat_phase_stamps.py): PhaseStamps, the helper splat_body calls, plus the side buffer's globals, their hand-over to
// a launch (attach_splat_stamps) and the entry point that sets them, accv_debug_splat_stamps.  Without the switch all of it is
// empty.  (The two SplatParams fields stay in splat_common.h: they are part of the kernel arguments.)
// Included once, from draw_heatmap.hip; needs splat_common.h.
#pragma once

namespace {

// ON = this build AND this instantiation carry stamps; otherwise every call below is empty
template <bool ON>
struct PhaseStamps {
    __device__ __forceinline__ void start() {}
    __device__ __forceinline__ void cull() {}
    __device__ __forceinline__ void table() {}
    __device__ __forceinline__ void accumulate() {}
    __device__ __forceinline__ void record(const SplatParams&, long long, int, int, int) {}
};

#ifdef ACCV_SPLAT_STAMPS
constexpr bool kSplatStampsBuilt = true;
__device__ __forceinline__ unsigned long long phase_stamp()   // 100 MHz constant clock; pinned in program order
{
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long v = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_sched_barrier(0);
    return v;
}
__device__ __forceinline__ unsigned xcc_id()
{
    unsigned v;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(v));
    return v;
}

// a stamp after each cull round, after each row table and after each accumulate loop; the record holds the wave's start,
// the time it spent in each of the three kinds of phase (summed over its rounds), the end of its last phase before the
// stores and the time after its last store was issued
template <>
struct PhaseStamps<true> {
    unsigned long long st_start = 0, st_prev = 0, st_cull = 0, st_table = 0, st_acc = 0;
    int rounds = 0;

    __device__ __forceinline__ unsigned long long lap()   // time since the previous stamp
    {
        const unsigned long long now = phase_stamp(), d = now - st_prev;
        st_prev = now;
        return d;
    }
    __device__ __forceinline__ void start() { st_start = st_prev = phase_stamp(); }
    __device__ __forceinline__ void cull()
    {
        st_cull += lap();
        ++rounds;
    }
    __device__ __forceinline__ void table() { st_table += lap(); }
    __device__ __forceinline__ void accumulate() { st_acc += lap(); }
    // after the last store: record `rec` = the tile's linear index, 8 x u64
    __device__ __forceinline__ void record(const SplatParams& p, long long rec, int lane, int n, int total_hits)
    {
        const unsigned long long done = phase_stamp();
        if (lane == 0 && p.stamps && rec < p.stamp_records) {   // lane 0 owns column tx0 < W and row ty0 < H: never left early
            unsigned long long* o = p.stamps + 8 * rec;
            o[0] = st_start;
            o[1] = st_cull;
            o[2] = st_table;
            o[3] = st_acc;
            o[4] = st_prev;
            o[5] = (unsigned long long)n;
            o[6] = done;
            o[7] = (unsigned long long)(unsigned)total_hits | ((unsigned long long)rounds << 16) | ((unsigned long long)xcc_id() << 32);
        }
    }
};

unsigned long long* g_splat_stamps = nullptr;   // diagnostic build: side buffer of the phase stamps (device memory)
long long g_splat_stamp_records = 0;
inline void attach_splat_stamps(SplatParams& p)
{
    p.stamps = g_splat_stamps;
    p.stamp_records = g_splat_stamp_records;
}
#else
constexpr bool kSplatStampsBuilt = false;
inline void attach_splat_stamps(SplatParams&) {}
#endif

}  // namespace

#ifdef ACCV_SPLAT_STAMPS
// diagnostic build only: fused-clear tile waves of the following splat_kernel launches write 8 x u64 per tile into `buffer`
// (device memory holding `records` records; nullptr switches the records off)
extern "C" void accv_debug_splat_stamps(void* buffer, long long records)
{
    g_splat_stamps = static_cast<unsigned long long*>(buffer);
    g_splat_stamp_records = buffer ? records : 0;
}
#endif
