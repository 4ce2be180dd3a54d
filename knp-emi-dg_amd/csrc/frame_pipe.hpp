// The frame pipeline of the samplers that hand dense frames to the host while the time loop goes on (grid.hip: voxel grids,
// surface.hip: membrane surfaces).  A sampler's kernels write one device frame; the frame is copied asynchronously into one of two
// pinned host buffers and an event follows on the context's stream; a fetch waits for the event of the oldest waiting frame only.
// Frame n lives in buffer n & 1, so at most two frames wait.  Per buffer three events: before the kernels, after them, after the copy.
//   const int b = P.begin(c, "...");      // -5: both buffers wait, otherwise the buffer; the `before` event is recorded
//   ... the sampler's kernels, on c->stream, writing P.frame ...
//   P.end(c, b);                          // `after` event, copy, `copied` event
#pragma once
#include "knpemi_internal.hpp"
#include <cstring>

struct FramePipe {
    size_t bytes = 0;               // of one frame
    void* frame = nullptr;          // device
    void* pinned[2] = {nullptr, nullptr};
    hipEvent_t ev[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    int64_t sampled = 0, fetched = 0;   // frames enqueued / handed out
    float sample_ms = 0.f, copy_ms = 0.f;   // of the last fetched frame

    // the device frame, both pinned buffers and the six events; false (and a cleared HIP error) when one of them fails: call release()
    bool alloc(size_t frame_bytes) {
        bytes = frame_bytes;
        bool ok = hipMalloc(&frame, bytes) == hipSuccess;
        for (int b = 0; b < 2 && ok; ++b) {
            ok = hipHostMalloc(&pinned[b], bytes) == hipSuccess;
            for (auto& e : ev[b]) ok = ok && hipEventCreate(&e) == hipSuccess;
        }
        if (!ok) (void)hipGetLastError();
        return ok;
    }
    void release() {
        hipFree(frame);
        frame = nullptr;
        for (int b = 0; b < 2; ++b) {
            if (pinned[b]) hipHostFree(pinned[b]);
            pinned[b] = nullptr;
            for (auto& e : ev[b]) {
                if (e) hipEventDestroy(e);
                e = nullptr;
            }
        }
    }
    // who: "knp_grid_sample" and the name of the fetch call, for the error text
    int begin(knp_ctx* c, const char* who, const char* fetch_call) {
        if (sampled - fetched >= 2) {
            c->err = std::string(who) + ": both frame buffers wait to be fetched (" + fetch_call + ")";
            return -5;
        }
        const int b = (int)(sampled & 1);
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipEventRecord(ev[b][0], c->stream));
        return b;
    }
    int end(knp_ctx* c, int b) {
        HIPCHK(c, hipEventRecord(ev[b][1], c->stream));
        HIPCHK(c, hipMemcpyAsync(pinned[b], frame, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipEventRecord(ev[b][2], c->stream));
        ++sampled;
        return 0;
    }
    // what: the shape the buffer must have, for the error text
    int fetch(knp_ctx* c, const char* who, const char* sample_call, const char* what, void* out, size_t out_bytes) {
        if (fetched >= sampled) { c->err = std::string(who) + ": no frame waits (" + sample_call + ")"; return -1; }
        if (out_bytes != bytes) { c->err = std::string(who) + ": the buffer must hold " + what; return -1; }
        const int b = (int)(fetched & 1);
        HIPCHK(c, host_event_sync(c, ev[b][2]));
        HIPCHK(c, hipEventElapsedTime(&sample_ms, ev[b][0], ev[b][1]));
        HIPCHK(c, hipEventElapsedTime(&copy_ms, ev[b][1], ev[b][2]));
        memcpy(out, pinned[b], out_bytes);
        ++fetched;
        return 0;
    }
};
