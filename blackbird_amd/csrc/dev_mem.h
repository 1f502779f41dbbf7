// dev_mem.h -- who owns the library's device memory, streams and events.  DevOwner: everything an engine, an arena or a trainer
// holds for its lifetime, given back by its destructor.  StagedOn<T>: a typed scratch buffer of one call, given back on scope exit.
// No HIP here: what touches the device comes in through DevOps (the HIP side: host_common.hip.h), so a stand-alone program can
// drive the same code over the C heap under a sanitizer (tests/test_dev_mem_cpu.py).
#pragma once
#include <cstddef>
#include <cstdio>
#include <vector>

struct DevOps { // the device side.  The functions that return int: 0, or the device's error code (what `why` puts into words)
    void *ctx;
    int (*alloc)(void *ctx, size_t bytes, void **out);
    void (*free)(void *ctx, void *p);
    int (*zero_async)(void *ctx, void *p, size_t bytes, void *stream);
    int (*copy)(void *ctx, void *dst, const void *src, size_t bytes); // either direction; returns when the bytes have arrived
    int (*stream_create)(void *ctx, void **out);
    void (*stream_destroy)(void *ctx, void *stream);
    int (*event_create)(void *ctx, bool timing, void **out);
    void (*event_destroy)(void *ctx, void *event);
    const char *(*why)(void *ctx, int rc);
    int (*fail)(void *ctx, const char *msg); // makes msg the thread's last error; returns the status the caller hands on
};

static inline int dev_fail(const DevOps &ops, const char *what, size_t bytes, bool with_bytes, int rc) {
    char msg[256];
    if (with_bytes) snprintf(msg, sizeof msg, "%s(%zu) failed: %s", what, bytes, ops.why(ops.ctx, rc));
    else snprintf(msg, sizeof msg, "%s failed: %s", what, ops.why(ops.ctx, rc));
    return ops.fail(ops.ctx, msg);
}

// Every function: 0, or what ops.fail answered after making the failure the thread's last error.  Nothing here reports twice and
// the destructor reports nothing, so after a create function that stops at its first failure the last error is that failure.
class DevOwner {
    const DevOps &ops_;
    std::vector<void *> allocs_, streams_, events_;

public:
    explicit DevOwner(const DevOps &ops) : ops_(ops) {}
    DevOwner(const DevOwner &) = delete;
    DevOwner &operator=(const DevOwner &) = delete;
    ~DevOwner() { // events, then memory, then streams
        for (void *ev : events_) ops_.event_destroy(ops_.ctx, ev);
        for (void *p : allocs_) ops_.free(ops_.ctx, p);
        for (void *s : streams_) ops_.stream_destroy(ops_.ctx, s);
    }
    // the stream the fills of alloc() run on: the first one made here (none yet: the null stream)
    void *fill_stream() const { return streams_.empty() ? nullptr : streams_[0]; }

    // count elements (none: 16 bytes), owned from here on; zero: filled with zeros asynchronously, on fill_stream()
    template <class T>
    int alloc(T *&p, size_t count, bool zero = true) {
        void *q = nullptr;
        const size_t bytes = count * sizeof(T);
        if (int rc = ops_.alloc(ops_.ctx, bytes ? bytes : 16, &q)) return dev_fail(ops_, "hipMalloc", bytes, true, rc);
        allocs_.push_back(q);
        if (zero && bytes)
            if (int rc = ops_.zero_async(ops_.ctx, q, bytes, fill_stream())) return dev_fail(ops_, "hipMemset", 0, false, rc);
        p = (T *)q;
        return 0;
    }
    // gives one allocation back before the owner dies (a buffer that is replaced by a larger one); false: p is not held here
    bool release(const void *p) {
        for (size_t i = 0; i < allocs_.size(); i++)
            if (p && allocs_[i] == p) {
                ops_.free(ops_.ctx, allocs_[i]);
                allocs_.erase(allocs_.begin() + (long)i);
                return true;
            }
        return false;
    }
    template <class S>
    int stream(S *&s) {
        void *q = nullptr;
        if (int rc = ops_.stream_create(ops_.ctx, &q)) return dev_fail(ops_, "hipStreamCreate", 0, false, rc);
        streams_.push_back(q);
        s = (S *)q;
        return 0;
    }
    template <class E>
    int event(E *&ev, bool timing) {
        void *q = nullptr;
        if (int rc = ops_.event_create(ops_.ctx, timing, &q)) return dev_fail(ops_, "hipEventCreate", 0, false, rc);
        events_.push_back(q);
        ev = (E *)q;
        return 0;
    }
};

// Scratch of one entry point: alloc(count) once, then whole-buffer or shorter copies; get() of a buffer never allocated is null.
template <class T>
class StagedOn {
    const DevOps &ops_;
    T *p_ = nullptr;
    size_t count_ = 0;
    int copy(void *dst, const void *src, size_t count, const char *what) const {
        if (count == ALL) count = count_;
        if (!p_ || count > count_) {
            char msg[128];
            snprintf(msg, sizeof msg, "%s of %zu elements, the staging buffer holds %zu", what, count, p_ ? count_ : (size_t)0);
            return ops_.fail(ops_.ctx, msg);
        }
        if (int rc = ops_.copy(ops_.ctx, dst, src, count * sizeof(T))) return dev_fail(ops_, "hipMemcpy", count * sizeof(T), true, rc);
        return 0;
    }

public:
    static constexpr size_t ALL = (size_t)-1;
    explicit StagedOn(const DevOps &ops) : ops_(ops) {}
    StagedOn(const StagedOn &) = delete;
    StagedOn &operator=(const StagedOn &) = delete;
    ~StagedOn() {
        if (p_) ops_.free(ops_.ctx, p_);
    }
    int alloc(size_t count) { // once per buffer
        if (p_) return ops_.fail(ops_.ctx, "staging buffer allocated twice");
        void *q = nullptr;
        const size_t bytes = count * sizeof(T);
        if (int rc = ops_.alloc(ops_.ctx, bytes ? bytes : 16, &q)) return dev_fail(ops_, "hipMalloc", bytes, true, rc);
        p_ = (T *)q;
        count_ = count;
        return 0;
    }
    T *get() const { return p_; }
    int from_host(const void *src, size_t count = ALL) { return copy(p_, src, count, "from_host"); }
    int to_host(void *dst, size_t count = ALL) const { return copy(dst, p_, count, "to_host"); }
};
