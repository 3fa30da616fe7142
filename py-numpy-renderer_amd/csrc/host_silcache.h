// host_silcache.h -- the silhouette cache of a scene (kernels_geometry.h, SilArgs).
//
// Which edges are on the silhouette and where their shadow quads stand in world space depends on the light and the
// geometry alone, so frames that only move the camera read both back.  The key is every byte the two steps read of the
// frame: the light's type, position AND direction (the light-facing test reads the position of a directional light
// too), compared as bytes.  The geometry is not in the key: commit() drops the cache whenever it rebuilds the static
// records.
//   * A key seen on two consecutive frames is captured: that frame's fused edge path also stores its entries, and its
//     stream copies the count to pinned memory and records an event.  Nobody waits: enqueues poll the event while a
//     capture is pending, and only a buffer whose event the HOST has seen complete is read -- so a reader on another
//     stream needs no hipStreamWaitEvent.
//   * Two buffers.  A buffer is captured into only when FREE: never read, or retired -- an event recorded on every
//     stream that read it, behind its last reader -- and those events seen complete.  If none is free, no capture.
// A frame makes two calls: choose_path() before it launches k_setup, and capture_launched() behind that launch when
// the path chosen was SIL_CAPTURE.  Nothing else changes a buffer's state or `pending`.
#pragma once

namespace {

struct SilKey { int32_t light_type, pad; double pos[3], dir[3]; };
inline SilKey sil_key(const mr::LightRec &l)
{
    SilKey key;
    std::memset(&key, 0, sizeof key);
    key.light_type = l.type;
    std::memcpy(key.pos, l.pos, sizeof key.pos);
    std::memcpy(key.dir, l.dir, sizeof key.dir);
    return key;
}

struct SilCache {
    enum State { FREE, CAPTURING, VALID, RETIRING };
    struct Buf {
        DevBuf quads, last;
        uint32_t cap = 0, count = 0;
        State state = FREE;
        SilKey key = {};
        hipEvent_t captured = nullptr;
        uint32_t *h_count = nullptr;              // pinned: the capture frame's silhouette count
        uint32_t readers = 0;                     // bit per frame slot that has enqueued a frame reading it
        uint64_t used = 0;                        // the scene's frame serial when it was last read
        hipEvent_t retire[MAX_SLOTS] = {};
        uint32_t retiring = 0;                    // RETIRING: the slots whose event is still awaited
    } buf[2];
    hipStream_t slot_stream[MAX_SLOTS] = {};      // the stream of every frame slot that has asked for a path
    SilKey last_key = {};
    bool have_last = false;
    int pending = 0;                              // buffers CAPTURING or RETIRING: only then are events polled
    Buf *capture = nullptr;                       // chosen by choose_path, until capture_launched
    int last_path = -1;                           // mr_debug_sil_cache: SIL_* of the last frame with shadows
    uint32_t last_entries = 0, captures = 0;

    void drop()                                   // (the device is idle: commit, mr_scene_clear)
    {
        for (Buf &b : buf) { b.state = FREE; b.readers = b.retiring = 0; b.count = 0; }
        have_last = false; pending = 0; capture = nullptr;
    }
    void release()
    {
        drop();
        for (Buf &b : buf) {
            b.quads.release(); b.last.release(); b.cap = 0;
            if (b.captured) (void)hipEventDestroy(b.captured);
            if (b.h_count) (void)hipHostFree(b.h_count);
            for (hipEvent_t &e : b.retire) { if (e) (void)hipEventDestroy(e); e = nullptr; }
            b.captured = nullptr; b.h_count = nullptr;
        }
    }
    int valid_buffers() const { return (buf[0].state == VALID) + (buf[1].state == VALID); }

    // A buffer to capture into: a free one; if there is none, the longest unused one starts to retire (and is free at once
    // when nobody has read it).
    Buf *free_buffer()
    {
        Buf *into = nullptr, *oldest = nullptr;
        for (Buf &b : buf) {
            if (b.state == FREE && !into) into = &b;
            if (b.state == VALID && (!oldest || b.used < oldest->used)) oldest = &b;
        }
        if (into || !oldest) return into;
        oldest->retiring = 0;
        for (int i = 0; i < MAX_SLOTS; ++i) {
            if (!(oldest->readers >> i & 1u)) continue;
            hipEvent_t &e = oldest->retire[i];
            if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
            if (hipEventRecord(e, slot_stream[i]) != hipSuccess) return nullptr;
            oldest->retiring |= 1u << i;
        }
        oldest->readers = 0;
        if (oldest->retiring) { oldest->state = RETIRING; pending += 1; return nullptr; }
        oldest->state = FREE;
        return oldest;
    }

    // Which path the edge half of this frame's k_setup takes: fills `sil`.  `enabled` is the frame's MR_SIL_CACHE; a frame
    // with several lights takes the fused edge path and leaves the cache, keyed on one light, as it is.
    void choose_path(bool enabled, int n_lights, int slot, hipStream_t stream, uint32_t quad_cap, uint64_t frame_serial,
                     const mr::LightRec &light, mr::SilArgs &sil)
    {
        sil = mr::SilArgs{};
        sil.mode = mr::SIL_FUSED;
        last_path = mr::SIL_FUSED; last_entries = 0;
        capture = nullptr;
        if (n_lights > 1) return;
        if (!enabled) { have_last = false; return; }
        slot_stream[slot] = stream;
        const SilKey key = sil_key(light);
        // what the host has seen complete since the last look: a capture becomes VALID, a retired buffer FREE
        if (pending) {
            for (Buf &b : buf) {
                if (b.state == CAPTURING && hipEventQuery(b.captured) == hipSuccess) {
                    b.count = *b.h_count;
                    b.state = b.count <= b.cap ? VALID : FREE;    // (an overflowed capture is discarded)
                    b.readers = 0;
                    pending -= 1;
                } else if (b.state == RETIRING) {
                    for (int i = 0; i < MAX_SLOTS; ++i)
                        if ((b.retiring >> i & 1u) && hipEventQuery(b.retire[i]) == hipSuccess) b.retiring &= ~(1u << i);
                    if (!b.retiring) { b.state = FREE; pending -= 1; }
                }
            }
        }
        const bool repeat = have_last && !std::memcmp(&last_key, &key, sizeof key);
        last_key = key; have_last = true;
        bool on_its_way = false;
        for (Buf &b : buf) {
            if (b.state != VALID && b.state != CAPTURING) continue;
            if (std::memcmp(&b.key, &key, sizeof key)) continue;
            if (b.state == CAPTURING) { on_its_way = true; continue; }
            sil.mode = mr::SIL_CACHED; sil.count = b.count;
            sil.quads = b.quads.as<mr::SilQuad>(); sil.last = b.last.as<uint32_t>();
            b.readers |= 1u << slot;
            b.used = frame_serial;
            last_path = mr::SIL_CACHED; last_entries = b.count;
            return;
        }
        if (!repeat || on_its_way) return;
        // a key worth keeping
        Buf *into = free_buffer();
        if (!into) return;
        if (!into->captured && hipEventCreateWithFlags(&into->captured, hipEventDisableTiming) != hipSuccess) return;
        if (!into->h_count && hipHostMalloc((void **)&into->h_count, sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) return;
        if (into->quads.ensure((size_t)quad_cap * sizeof(mr::SilQuad)) != hipSuccess) return;
        if (into->last.ensure((size_t)quad_cap * sizeof(uint32_t)) != hipSuccess) return;
        into->cap = quad_cap; into->key = key;
        sil.mode = mr::SIL_CAPTURE; sil.count = quad_cap;
        sil.quads = into->quads.as<mr::SilQuad>(); sil.last = into->last.as<uint32_t>();
        last_path = mr::SIL_CAPTURE;
        captures += 1;
        capture = into;
    }

    // The k_setup of a frame on the SIL_CAPTURE path has been launched on `stream`: the count follows on that stream; the
    // buffer is read once the host has seen the event complete.
    int capture_launched(const uint32_t *d_count, hipStream_t stream)
    {
        hipError_t e = hipMemcpyAsync(capture->h_count, d_count, sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipEventRecord(capture->captured, stream);
        if (e != hipSuccess) return fail(MR_E_DEVICE, std::string("silhouette capture: ") + hipGetErrorString(e));
        capture->state = CAPTURING;
        pending += 1;
        capture = nullptr;
        return MR_OK;
    }
};

}  // namespace
