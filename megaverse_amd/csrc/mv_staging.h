// megaverse_amd/csrc/mv_staging.h -- the two ways per-env values travel from the caller's host memory to the device in stream order.  Both
// copy the caller's bytes into pinned memory of their own before they return, so the caller's array is free again at once; they differ in when that pinned
// memory may be written again.  Neither knows a gym: what they need is passed in.  Included by mv_api_internal.h, behind fail() and HIP_TRY.
#pragma once

namespace mvapi {

// Pool: for attachments that persist and whose setter never waits on the host (step masks, draw masks, episode budgets).  Pinned buffers of one byte size,
// each with the event recorded behind the copy that read it; a buffer is free again once that event has completed.
struct StagingPool {
    struct Buffer { void *host; hipEvent_t copied; };
    std::vector<Buffer> buffers;

    // a buffer nothing in flight reads: one whose copy has completed (asked, not waited for), else a new one.  The caller fills out->host, enqueues its
    // copies and records out->copied behind the last of them.
    int take(size_t bytes, const char *who, Buffer *&out)
    {
        out = nullptr;
        for (Buffer &b : buffers)
            if (hipEventQuery(b.copied) == hipSuccess) { out = &b; break; }
        (void)hipGetLastError();   // (hipErrorNotReady of the queries, on every path: it must not surface in a later call's hipGetLastError)
        if (out) return 0;
        Buffer b{nullptr, nullptr};
        HIP_TRY(hipHostMalloc(&b.host, bytes, hipHostMallocDefault));
        {
            hipError_t e_ = hipEventCreateWithFlags(&b.copied, hipEventDisableTiming);
            if (e_ != hipSuccess) { (void)hipHostFree(b.host); return fail(std::string(who) + ": hipEventCreate: " + hipGetErrorString(e_)); }
        }
        buffers.push_back(b);
        out = &buffers.back();
        return 0;
    }

    void release()
    {
        for (Buffer &b : buffers) {
            if (b.copied) (void)hipEventDestroy(b.copied);
            if (b.host) (void)hipHostFree(b.host);
        }
        buffers.clear();
    }
};

// Pair: for one-shot calls (fork / resample / env-store maps, reset masks, seed words).  Two device halves, two pinned halves and an event per half, allocated
// at the first use; the calls take the halves in turn, and a call may wait on the host for the call before last -- whose copy and launch are long done.
// Nothing is cleared: a half is written before it is read.
struct StagingPair {
    uint8_t *device = nullptr, *host = nullptr;   // [2][bytes] each
    hipEvent_t copied[2] = {nullptr, nullptr};
    unsigned long long uses = 0;

    // src's bytes -> the device half whose turn it is, on stream s.  The half's event is recorded here, behind the copy, with the use that is counted here --
    // whatever becomes of the launch that follows, the event of this use exists -- and mark() records it again behind the launch that read the half.
    template <class T>
    int stage(const T *src, size_t bytes, hipStream_t s, const T **device_half)
    {
        if (!device) {
            hipError_t e_ = hipMalloc((void **)&device, 2 * bytes);
            if (e_ == hipSuccess) e_ = hipHostMalloc((void **)&host, 2 * bytes, hipHostMallocDefault);
            for (hipEvent_t &e : copied)
                if (e_ == hipSuccess) e_ = hipEventCreateWithFlags(&e, hipEventDisableTiming);
            if (e_ != hipSuccess) { release(); return fail("host staging: allocating two halves of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e_)); }
        }
        const int b = (int)(uses & 1ull);
        // (the copy and the launch that used this half two calls ago: long done -- the staging is the host's to write again, the device half the stream's)
        if (uses >= 2) HIP_TRY(hipEventSynchronize(copied[b]));
        std::memcpy(host + (size_t)b * bytes, src, bytes);
        HIP_TRY(hipMemcpyAsync(device + (size_t)b * bytes, host + (size_t)b * bytes, bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(copied[b], s));
        *device_half = reinterpret_cast<const T *>(device + (size_t)b * bytes);
        ++uses;
        return 0;
    }

    // behind the launch that read the half stage() gave out last
    int mark(hipStream_t s)
    {
        HIP_TRY(hipEventRecord(copied[(int)((uses - 1) & 1ull)], s));
        return 0;
    }

    void release()
    {
        if (device) (void)hipFree(device);
        if (host) (void)hipHostFree(host);
        for (hipEvent_t &e : copied) { if (e) (void)hipEventDestroy(e); e = nullptr; }
        device = host = nullptr;
        uses = 0;
    }
};

}  // namespace mvapi
