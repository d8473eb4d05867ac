// What the detection decoders share (center_decode.hip, box_decode.hip, rotated_nms.hip, and the output checks of
// query_decode.hip): the workgroup geometry of the wave-block walk, the plane table of "up to 8 maps read in place", the
// checks of the output rows, and the first half of phase 3 — output slots from the kept masks.  Phase 2, the suppression
// walk, is NOT here: each kernel keeps its own (DESIGN, "Two kernels, one walk").  Nor are the compaction loop and the
// padding tail of phase 3: behind a template that takes the operator's row writers every kernel compiled to other
// instructions, so they stay spelled out in each.
//
// Like accv_numeric.h this header carries no file-scope `#pragma clang fp contract`; nothing in it rounds.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "accv_common.h"
#include "accv_numeric.h"

namespace accv_det {

// ------------------------------------------------------------------------------------------------------------ geometry
// One workgroup of kThreads lanes per row of at most kMaxSlots slots (peaks or boxes); the slots are walked in chunks of
// kThreads, a lane per slot, so a lane owns up to kChunks slots and keeps one `alive` bit for each.  A block is kWave
// consecutive slots = one wave of one chunk.  An operator file states kWave and kThreads itself, next to its kernel (its
// tests read them there), and takes everything that follows from them from here.
template <int kMaxSlots, int kThreads, int kWave>
struct Geometry {
    static constexpr int kWaves = kThreads / kWave;
    static constexpr int kChunks = kMaxSlots / kThreads;   // chunks a workgroup walks at most
    static constexpr int kBlocks = kMaxSlots / kWave;      // NMS blocks at most
    static_assert(kMaxSlots % kThreads == 0 && kChunks <= 32, "a lane keeps one alive bit per chunk");

    // Phase 3, first half.  s_keep[j] holds the kept mask of block j (0 for a block that does not exist); the output slot
    // of a kept slot is the popcount of the kept masks of the blocks before it plus that of the lower lanes of its own.
    // Returns the number of kept slots, and in base[c] the output slot of lane 0 of my wave's block of chunk c.
    __device__ static inline int slot_bases(const unsigned long long* s_keep, int (&base)[kChunks])
    {
        const int wave = threadIdx.x / kWave;
        int total = 0;
#pragma unroll
        for (int j = 0; j < kBlocks; ++j) {
            if (j % kWaves == wave) base[j / kWaves] = total;
            total += __popcll(s_keep[j]);
        }
        return total;
    }
};

__host__ __device__ inline long long clamp_size(long long v, long long hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// --------------------------------------------------------------------------------------------------------- plane table
// The maps of a head are read in place, never concatenated: chan[c] is the plane of concatenated channel c in frame 0 of
// its map and chan_count[c] the channel count of that map, so channel c at `cell` of frame f is element
// f * chan_count[c] * plane + cell from chan[c].  fill_planes builds one row of that table (max_channels entries, the
// unused ones null) from a row of map pointers; a map without channels is passed over and may be null.  `of` follows
// "map %d" in the messages (" of task 2", or "").  The caller has checked that the channel counts are not negative and add
// up to at most max_channels.
inline int fill_planes(const char* who, const char* of, const void* const* maps, const int* channels, int num_maps, long long plane,
                       uintptr_t map_size, int max_channels, const void** chan, unsigned char* chan_count)
{
    int c = 0;
    for (int i = 0; i < num_maps; ++i) {
        if (channels[i] == 0) continue;
        if (!maps[i]) return accv::fail(ACCV_EINVAL, "%s: map %d%s is null", who, i, of);
        if (reinterpret_cast<uintptr_t>(maps[i]) & (map_size - 1u))
            return accv::fail(ACCV_EINVAL, "%s: map %d%s is not aligned to its element size", who, i, of);
        for (int local = 0; local < channels[i]; ++local, ++c) {
            chan[c] = static_cast<const char*>(maps[i]) + (size_t)local * (size_t)plane * map_size;
            chan_count[c] = (unsigned char)channels[i];
        }
    }
    for (; c < max_channels; ++c) chan[c] = nullptr, chan_count[c] = 0;
    return ACCV_OK;
}

// concatenated channel c at `cell` of frame f, widened exactly
__host__ __device__ inline float channel_at(const void* const* chan, const unsigned char* chan_count, long long plane, int dt, int c,
                                            long long f, long long cell)
{
    return accv::load_any(chan[c], f * (long long)chan_count[c] * plane + cell, dt);
}

// --------------------------------------------------------------------------------------------------------- output rows
// The rows every decoder writes: boxes, scores and source (4-byte elements), labels and sizes (8-byte), and the extras
// (4-byte) of an operator that has them; `extras` counts only with has_extras.  Three checks, so that an operator with a
// check of its own between them keeps its order.
inline int outputs_present(const char* who, const void* boxes, const void* scores, const void* labels, const void* source,
                           const void* sizes, bool has_extras = false, const void* extras = nullptr)
{
    if (!boxes || !scores || !labels || !source || !sizes || (has_extras && !extras)) return accv::fail(ACCV_EINVAL, "%s: null output pointer", who);
    return ACCV_OK;
}

inline int outputs_aligned(const char* who, const void* boxes, const void* scores, const void* labels, const void* source,
                           const void* sizes, bool has_extras = false, const void* extras = nullptr)
{
    if ((reinterpret_cast<uintptr_t>(boxes) | reinterpret_cast<uintptr_t>(scores) | reinterpret_cast<uintptr_t>(source) |
         (has_extras ? reinterpret_cast<uintptr_t>(extras) : 0)) & 3u)
        return accv::fail(ACCV_EINVAL, "%s: a 4-byte output is not aligned to its element size", who);
    if ((reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(sizes)) & 7u)
        return accv::fail(ACCV_EINVAL, "%s: labels and sizes must be 8-byte aligned", who);
    return ACCV_OK;
}

inline int grid_fits(const char* who, long long groups)
{
    if (groups > accv::kGridLimit) return accv::fail(ACCV_EINVAL, "%s: %lld workgroups exceed the grid limit", who, groups);
    return ACCV_OK;
}

// the three in the order of an operator that has nothing between them; `groups` is the x extent of its grid
inline int check_outputs(const char* who, long long groups, const void* boxes, const void* scores, const void* labels, const void* source,
                         const void* sizes, bool has_extras = false, const void* extras = nullptr)
{
    if (int rc = outputs_present(who, boxes, scores, labels, source, sizes, has_extras, extras)) return rc;
    if (int rc = outputs_aligned(who, boxes, scores, labels, source, sizes, has_extras, extras)) return rc;
    return grid_fits(who, groups);
}

}  // namespace accv_det
