"""The owner of the library's device memory, streams and events (csrc/dev_mem.h: DevOwner) and the staging buffer of an entry
point (StagedOn<T>), driven by a stand-alone program over the C heap under AddressSanitizer + UBSan.

The device is the C heap: an allocation is a malloc block of exactly the bytes asked for, a stream or an event a block of one
byte, so anything kept after its owner died is a leak at exit, anything given back twice is counted (and would be a double free),
and a copy past a buffer's end is a heap overflow.  Every device call that can fail is numbered; the program lets the i-th fail,
for every i of a create sequence shaped like bb_create's (a stream, events, allocations with and without the zero fill, a second
stream), and asks after each run what the issue of a leaking create function asks: failure reported, the error text the first
failure's, nothing alive, nothing freed twice."""
import os
import shutil
import subprocess

import pytest

from blackbird_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blackbird_amd", "csrc")

PROGRAM = r"""
#include "dev_mem.h"
#include <cassert>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <set>
#include <string>
#include <utility>
#include <vector>

struct Heap {
    int calls = 0, fail_at = 0; // device calls that can fail, counted; the fail_at-th one fails (0: none)
    std::set<void *> allocs, streams, events; // alive
    int twice = 0, frees = 0, reports = 0;
    std::vector<size_t> asked, copied;                // bytes of every alloc / copy
    std::vector<std::pair<size_t, void *>> zeroed;    // bytes and stream of every zero fill
    std::string order, last;                          // 'e' / 'a' / 's' per object given back; the thread's last error
    char text[64];
    int next() { return ++calls == fail_at ? 1000 + calls : 0; }
    bool clean() const { return allocs.empty() && streams.empty() && events.empty() && twice == 0; }
};
static void *make(std::set<void *> &live, size_t bytes) {
    void *p = malloc(bytes);
    live.insert(p);
    return p;
}
static void give_back(Heap *h, std::set<void *> &live, void *p, char tag) {
    h->order += tag;
    if (!live.erase(p)) {
        h->twice++; // (not freed again: the count is the finding)
        return;
    }
    free(p);
}
static int h_alloc(void *c, size_t bytes, void **out) {
    Heap *h = (Heap *)c;
    h->asked.push_back(bytes);
    if (int rc = h->next()) return rc;
    *out = make(h->allocs, bytes);
    return 0;
}
static void h_free(void *c, void *p) { ((Heap *)c)->frees++; give_back((Heap *)c, ((Heap *)c)->allocs, p, 'a'); }
static int h_zero(void *c, void *p, size_t bytes, void *stream) {
    Heap *h = (Heap *)c;
    h->zeroed.push_back({bytes, stream});
    if (int rc = h->next()) return rc;
    memset(p, 0, bytes);
    return 0;
}
static int h_copy(void *c, void *dst, const void *src, size_t bytes) {
    Heap *h = (Heap *)c;
    h->copied.push_back(bytes);
    if (int rc = h->next()) return rc;
    memcpy(dst, src, bytes);
    return 0;
}
static int h_stream(void *c, void **out) {
    Heap *h = (Heap *)c;
    if (int rc = h->next()) return rc;
    *out = make(h->streams, 1);
    return 0;
}
static void h_stream_destroy(void *c, void *s) { give_back((Heap *)c, ((Heap *)c)->streams, s, 's'); }
static int h_event(void *c, bool, void **out) {
    Heap *h = (Heap *)c;
    if (int rc = h->next()) return rc;
    *out = make(h->events, 1);
    return 0;
}
static void h_event_destroy(void *c, void *e) { give_back((Heap *)c, ((Heap *)c)->events, e, 'e'); }
static const char *h_why(void *c, int rc) {
    Heap *h = (Heap *)c;
    snprintf(h->text, sizeof h->text, "injected failure #%d", rc - 1000);
    return h->text;
}
static int h_fail(void *c, const char *msg) {
    Heap *h = (Heap *)c;
    h->last = msg;
    h->reports++;
    return 3; // (BB_ERR_HIP's part)
}
static DevOps ops_over(Heap *h) {
    return DevOps{h, h_alloc, h_free, h_zero, h_copy, h_stream, h_stream_destroy, h_event, h_event_destroy, h_why, h_fail};
}

// ---- a create function of bb_create's shape: k = 5 allocations, s = 2 streams, v = 3 events ----
struct Thing {
    DevOwner own;
    void *stream = nullptr, *second = nullptr, *ev[3] = {nullptr, nullptr, nullptr};
    float *f = nullptr;
    double *d = nullptr;
    uint8_t *raw = nullptr;
    int32_t *none = nullptr;
    struct Wide { char c[24]; } *wide = nullptr;
    explicit Thing(const DevOps &ops) : own(ops) {}
};
static int thing_create(const DevOps &ops, Thing **out) {
    std::unique_ptr<Thing> t(new Thing(ops));
    if (t->own.stream(t->stream) || t->own.event(t->ev[0], false) || t->own.event(t->ev[1], false)) return 3;
    bool bad = t->own.alloc(t->f, 7) || t->own.alloc(t->raw, 33, false);
    bad = bad || t->own.alloc(t->d, 3, true);
    if (bad) return 3;
    if (int rc = t->own.alloc(t->none, 0)) return rc;           // nothing asked for: 16 bytes, and nothing to fill
    if (int rc = t->own.event(t->ev[2], true)) return rc;       // (the order of creation is not the order of destruction)
    if (int rc = t->own.alloc(t->wide, 2)) return rc;
    if (int rc = t->own.stream(t->second)) return rc;
    *out = t.release();
    return 0;
}

static void test_create_and_destroy() {
    Heap h;
    const DevOps ops = ops_over(&h);
    Thing *t = nullptr;
    assert(thing_create(ops, &t) == 0 && t && h.reports == 0);
    // byte counts: count * sizeof(T); none asked for: 16
    const std::vector<size_t> want = {7 * sizeof(float), 33, 3 * sizeof(double), 16, 2 * 24};
    assert(h.asked == want);
    // the zero fill exactly where the flag says so (and where there is something to fill), on the owner's first stream
    assert(h.zeroed.size() == 3 && t->stream && t->own.fill_stream() == t->stream && t->second != t->stream);
    assert(h.zeroed[0] == std::make_pair(7 * sizeof(float), t->stream) && h.zeroed[1] == std::make_pair(3 * sizeof(double), t->stream) &&
           h.zeroed[2] == std::make_pair((size_t)48, t->stream));
    for (int i = 0; i < 7; i++) assert(t->f[i] == 0.f);
    assert(h.allocs.size() == 5 && h.streams.size() == 2 && h.events.size() == 3);
    assert(h.calls == 5 + 3 + 2 + 3); // allocations, their fills, streams, events
    delete t;
    assert(h.order == "eeeaaaaass" && h.clean()); // events, then memory, then streams
    {
        DevOwner lone(ops); // without a stream of its own the fills go to the null stream
        char *p = nullptr;
        assert(lone.fill_stream() == nullptr && lone.alloc(p, 5) == 0 && h.zeroed.back() == std::make_pair((size_t)5, (void *)nullptr));
    }
    assert(h.clean());
}

static void test_every_failure() {
    Heap ok;
    Thing *t = nullptr;
    {
        const DevOps ops = ops_over(&ok);
        assert(thing_create(ops, &t) == 0);
        delete t;
    }
    const int total = ok.calls;
    assert(total >= 5 + 2 + 3);
    for (int i = 1; i <= total; i++) {
        Heap h;
        h.fail_at = i;
        const DevOps ops = ops_over(&h);
        Thing *out = nullptr;
        assert(thing_create(ops, &out) == 3 && out == nullptr); // reported ...
        char first[64];
        snprintf(first, sizeof first, "failed: injected failure #%d", i);
        assert(h.reports == 1 && h.last.find(first) != std::string::npos); // ... once, and the text is the first failure's ...
        assert(h.calls == i);                                              // (nothing was tried after it)
        assert(h.clean());                                                 // ... nothing alive, nothing given back twice
    }
    { // the text of a failed allocation: dalloc's
        Heap h;
        h.fail_at = 6; // calls 1 to 3: the stream and two events; 4 and 5: `f` and its fill; 6: `raw`
        const DevOps ops = ops_over(&h);
        Thing *out = nullptr;
        assert(thing_create(ops, &out) == 3 && h.last == "hipMalloc(33) failed: injected failure #6" && h.clean());
        Heap g;
        g.fail_at = 4;
        const DevOps gops = ops_over(&g);
        assert(thing_create(gops, &out) == 3 && g.last == "hipMalloc(28) failed: injected failure #4" && g.clean());
        Heap z;
        z.fail_at = 8; // 7: `d`; 8: its fill
        const DevOps zops = ops_over(&z);
        assert(thing_create(zops, &out) == 3 && z.last == "hipMemset failed: injected failure #8" && z.clean());
    }
}

static void test_release() {
    Heap h;
    const DevOps ops = ops_over(&h);
    int local = 0;
    {
        DevOwner own(ops);
        int32_t *p = nullptr, *q = nullptr;
        assert(own.alloc(p, 4, false) == 0 && own.alloc(q, 4, false) == 0 && h.allocs.size() == 2);
        assert(own.release(p) && h.frees == 1 && h.allocs.size() == 1 && h.allocs.count(q));
        assert(!own.release(p) && !own.release(&local) && !own.release(nullptr) && h.frees == 1); // refused, the heap untouched
        int32_t *r = nullptr;
        assert(own.alloc(r, 9, false) == 0); // the grow-and-replace of the trainer's scratch
        q[3] = 1;
        r[8] = 2;
    }
    assert(h.frees == 3 && h.clean() && h.reports == 0); // q and r by the destructor, p not again
}

static int staged_path(const DevOps &ops, Heap &h, int leave_at) {
    StagedOn<double> s(ops);
    assert(s.get() == nullptr);
    if (int rc = s.alloc(5)) return rc;
    assert(h.asked.back() == 5 * sizeof(double) && h.allocs.size() == 1);
    if (leave_at == 1) return -1;
    const double src[5] = {1, 2, 3, 4, 5};
    if (int rc = s.from_host(src)) return rc; // the whole buffer
    assert(h.copied.back() == 5 * sizeof(double));
    if (leave_at == 2) return -2;
    double back[3] = {0, 0, 0};
    if (int rc = s.to_host(back, 3)) return rc;
    assert(h.copied.back() == 3 * sizeof(double) && back[0] == 1 && back[2] == 3);
    return 0;
}

static void test_staged() {
    Heap h;
    const DevOps ops = ops_over(&h);
    assert(staged_path(ops, h, 0) == 0 && h.clean());
    assert(staged_path(ops, h, 1) == -1 && h.clean()); // freed on every way out
    assert(staged_path(ops, h, 2) == -2 && h.clean());
    for (int i = 1; i <= 3; i++) { // a failed allocation, a failed copy in, a failed copy out
        Heap g;
        g.fail_at = i;
        const DevOps gops = ops_over(&g);
        assert(staged_path(gops, g, 0) == 3 && g.reports == 1 && g.clean());
        char first[64];
        snprintf(first, sizeof first, "failed: injected failure #%d", i);
        assert(g.last.find(first) != std::string::npos);
        if (i == 1) assert(g.last == "hipMalloc(40) failed: injected failure #1");
    }
    {
        StagedOn<double> s(ops);
        double six[6] = {0, 0, 0, 0, 0, 0};
        const size_t copies = h.copied.size();
        assert(s.from_host(six, 1) == 3 && h.copied.size() == copies); // never allocated: refused
        assert(s.alloc(5) == 0);
        const int reports = h.reports;
        assert(s.from_host(six, 6) == 3 && s.to_host(six, 6) == 3 && h.reports == reports + 2 && h.copied.size() == copies); // more than it holds
        assert(s.from_host(six, 5) == 0 && s.to_host(six, 0) == 0 && h.copied.back() == 0);
        assert(s.alloc(5) == 3 && h.allocs.size() == 1); // once per buffer
    }
    assert(h.clean());
    {
        StagedOn<int32_t> none(ops);
        int32_t x = 7;
        assert(none.alloc(0) == 0 && h.asked.back() == 16 && none.get() && none.from_host(&x) == 0 && h.copied.back() == 0);
        assert(none.from_host(&x, 1) == 3);
        struct Rec { char c[12]; };
        StagedOn<Rec> recs(ops);
        assert(recs.alloc(3) == 0 && h.asked.back() == 36);
        Rec r[3];
        memset(r, 5, sizeof r);
        assert(recs.from_host(r) == 0 && h.copied.back() == 36 && recs.to_host(r, 2) == 0 && h.copied.back() == 24);
    }
    assert(h.clean());
}

int main() {
    test_create_and_destroy();
    test_every_failure();
    test_release();
    test_staged();
    puts("dev_mem host ok");
    return 0;
}
"""


def test_owner_and_staging_buffer_under_address_and_ub_sanitizers(tmp_path):
    if _lib.lib().bb_device_count() > 0:
        pytest.skip("GPU present: sanitizer builds run on machines without one")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "dev_mem_host.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "dev_mem_host")
    cmd = [hipcc, "-std=c++17", "-O1", "-g", "-UNDEBUG", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
           "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, str(src)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "dev_mem host ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])


def test_the_library_allocates_through_the_owner_only():
    """A raw hipMalloc / hipFree / stream or event creation stands in the HIP side of dev_mem.h alone (csrc/host_common.hip.h)."""
    import re
    raw = re.compile(r"\bhip(Malloc|Free|StreamCreate\w*|EventCreate\w*)\s*\(")
    found = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".h", ".hip")):
            code = re.sub(r"//.*", "", open(os.path.join(CSRC, name)).read())
            if raw.search(code):
                found[name] = len(raw.findall(code))
    assert found == {"host_common.hip.h": 5}, found
