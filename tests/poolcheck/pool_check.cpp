// The block cache behind the library's device memory and pinned host memory (csrc/trc_pool.h) driven through a fake backend: the
// size classes, reuse, the caps, which block is evicted, the retry after a refused allocation, the device a block is kept under,
// the one wait before a block is kept, and the books after eight threads have used one cache.  A program of its own (`make
// poolcheck` builds it with -fsanitize=address,undefined, `make poolcheck-tsan` with -fsanitize=thread; tests/test_pool_host.py
// runs both): prints one line per violated property and returns their number.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <random>
#include <set>
#include <thread>
#include <vector>
#include "../../tracer_amd/csrc/trc_pool.h"

static std::atomic<int> bad(0);
#define EXPECT(cond, ...) do { if (!(cond)) { if (++bad <= 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const size_t KiB = (size_t)1 << 10, MiB = (size_t)1 << 20, GiB = (size_t)1 << 30;

// what the fake backend has been asked: blocks are 1 byte of malloc whatever their size
struct Fake {
    std::mutex mu;
    std::set<void *> out;                 // handed out and not released
    std::vector<void *> released;         // in order
    std::vector<size_t> asked;            // sizes of the allocations that were tried, in order
    long allocs = 0, releases = 0, quiesces = 0, foreign = 0;      // (allocs: those that gave a block)
    std::atomic<int> fail_next{0};        // refuse this many allocations
    std::atomic<int> dev{0};
    ~Fake() { for (void *p : out) std::free(p); }
    void *make() {                        // a block of the backend's that no cache has seen
        std::lock_guard<std::mutex> g(mu);
        void *p = std::malloc(1);
        out.insert(p);
        return p;
    }
};
struct FakeBackend {
    Fake *f;
    void *alloc(size_t bytes) {
        {
            std::lock_guard<std::mutex> g(f->mu);
            f->asked.push_back(bytes);
        }
        int k = f->fail_next.load();
        while (k > 0 && !f->fail_next.compare_exchange_weak(k, k - 1)) {}
        if (k > 0) return nullptr;
        void *p = f->make();
        std::lock_guard<std::mutex> g(f->mu);
        ++f->allocs;
        return p;
    }
    void release(void *p) {
        std::lock_guard<std::mutex> g(f->mu);
        ++f->releases;
        if (!f->out.erase(p)) { ++f->foreign; return; }
        f->released.push_back(p);
        std::free(p);
    }
    void quiesce() { std::lock_guard<std::mutex> g(f->mu); ++f->quiesces; }
    int device() { return f->dev.load(); }
};
typedef trc_block_cache<FakeBackend> Cache;

// the policies of the library: dev_cache (trc_host.h) and g_host_cache (trc_scene.hip)
static const trc_pool_policy DEVICE = {128 * MiB, 2 * GiB, 2 * GiB, true, true};
static const trc_pool_policy HOST = {SIZE_MAX, 4 * GiB, 0, false, false};

static void check_classes() {
    auto at = [](size_t b) {
        const size_t c = trc_pool_class(b);
        EXPECT(c >= b, "class(%zu) = %zu", b, c);
        if (b > 256) EXPECT(c - b <= b / 8, "class(%zu) = %zu", b, c);
        else EXPECT(c == 256, "class(%zu) = %zu", b, c);
        EXPECT(trc_pool_class(c) == c, "class(%zu) = %zu, class of that %zu", b, c, trc_pool_class(c));
    };
    long n = 0;
    for (int k = 3; k < 46; ++k)
        for (size_t j = 0; j <= 8; ++j)
            for (long d = -3; d <= 3; ++d) {
                const long long b = (long long)(((size_t)1 << k) + j * (((size_t)1 << k) >> 3)) + d;
                if (b >= 1 && b < (1ll << 46)) { at((size_t)b); ++n; }
            }
    size_t prev = 0;
    for (size_t b = 1; b <= 70000; ++b) {
        at(b);
        EXPECT(trc_pool_class(b) >= prev, "class(%zu) = %zu after %zu", b, trc_pool_class(b), prev);
        prev = trc_pool_class(b);
    }
    EXPECT(trc_pool_class(1) == 256 && trc_pool_class(257) == 288 && trc_pool_class(1000) == 1024 && trc_pool_class(MiB + 1) == MiB + MiB / 8,
           "%zu %zu %zu %zu", trc_pool_class(1), trc_pool_class(257), trc_pool_class(1000), trc_pool_class(MiB + 1));
    std::printf("classes: %ld sizes on the grid\n", n);
}

static void check_device_policy() {
    {   // a freed block is the next one of its class, with nothing asked of the backend
        Fake f; Cache c(DEVICE, true, FakeBackend{&f});
        void *p = c.alloc(1000);
        EXPECT(p && f.asked.back() == 1024 && c.live_blocks() == 1, "asked %zu", f.asked.back());
        EXPECT(c.free(p) == TRC_POOL_KEPT && c.idle_classed_bytes() == 1024 && c.live_blocks() == 0, "idle %zu", c.idle_classed_bytes());
        void *q = c.alloc(970);
        EXPECT(q == p && f.allocs == 1 && f.asked.size() == 1 && f.quiesces == 1 && f.releases == 0, "allocs %ld quiesces %ld", f.allocs, f.quiesces);
        EXPECT(c.idle_blocks() == 0 && c.idle_classed_bytes() == 0 && c.live_blocks() == 1, "idle %zu", c.idle_blocks());
        void *r = c.alloc(970);           // while q is live: another block
        EXPECT(r && r != q && f.allocs == 2, "allocs %ld", f.allocs);
        c.free(q); c.free(r); c.trim();
        EXPECT(f.out.empty() && f.releases == 2 && c.idle_blocks() == 0, "releases %ld", f.releases);
    }
    {   // the key is the device current at the allocation, not at the free
        Fake f; Cache c(DEVICE, true, FakeBackend{&f});
        void *p = c.alloc(1000);
        f.dev = 1;
        EXPECT(c.free(p) == TRC_POOL_KEPT && c.idle_blocks(0, 1024) == 1 && c.idle_blocks(1, 1024) == 0, "kept under device 1");
        void *q = c.alloc(1000);
        EXPECT(q && q != p && f.allocs == 2 && c.idle_blocks(0, 1024) == 1, "device 1 was handed the block of device 0");
        f.dev = 0;
        void *r = c.alloc(1000);
        EXPECT(r == p && f.allocs == 2, "allocs %ld", f.allocs);
        c.free(q); c.free(r); c.trim();
    }
    {   // exact blocks: not rounded, kept by their size, the oldest makes room
        Fake f; Cache c(DEVICE, true, FakeBackend{&f});
        const size_t M = 900 * MiB;
        void *a = c.alloc(M + 7), *b = c.alloc(M + 8), *d = c.alloc(M + 9);
        EXPECT(f.asked.size() == 3 && f.asked[0] == M + 7 && f.asked[1] == M + 8 && f.asked[2] == M + 9, "an exact size was rounded");
        EXPECT(c.free(a) == TRC_POOL_KEPT && c.free(b) == TRC_POOL_KEPT && f.releases == 0 && c.idle_exact_bytes() == 2 * M + 15, "idle %zu", c.idle_exact_bytes());
        EXPECT(c.free(d) == TRC_POOL_KEPT, "the third block was not kept");
        EXPECT(f.releases == 1 && f.released.size() == 1 && f.released[0] == a, "releases %ld", f.releases);
        EXPECT(c.idle_exact_bytes() == 1800 * MiB + 17 && c.idle_classed_bytes() == 0 && c.idle_blocks() == 2 && f.quiesces == 3, "idle %zu", c.idle_exact_bytes());
        EXPECT(c.alloc(M + 8) == b && f.allocs == 3 && c.alloc(M + 7) && f.allocs == 4, "allocs %ld", f.allocs);
        EXPECT(c.idle_exact_bytes() == M + 9, "idle %zu", c.idle_exact_bytes());
    }
    {   // a block beyond the cap is never kept
        Fake f; Cache c(DEVICE, true, FakeBackend{&f});
        void *p = c.alloc(3 * GiB);
        EXPECT(f.asked.back() == 3 * GiB && c.free(p) == TRC_POOL_RELEASED && f.releases == 1 && f.quiesces == 0 && c.idle_blocks() == 0, "a 3 GiB block was kept");
    }
    {   // the cap of the classed blocks
        Fake f; Cache c(DEVICE, true, FakeBackend{&f});
        std::vector<void *> ps;
        for (int i = 0; i < 20; ++i) ps.push_back(c.alloc(128 * MiB));
        int kept = 0, released = 0;
        for (void *p : ps) { const trc_pool_freed r = c.free(p); kept += r == TRC_POOL_KEPT; released += r == TRC_POOL_RELEASED; }
        EXPECT(kept == 16 && released == 4 && f.releases == 4, "kept %d released %d", kept, released);
        EXPECT(c.idle_classed_bytes() == 2 * GiB && c.idle_exact_bytes() == 0 && c.idle_blocks() == 16 && f.quiesces == 16, "idle %zu quiesces %ld", c.idle_classed_bytes(), f.quiesces);
    }
    {   // a refused allocation: everything idle, of every device, goes back, and the request is made once more
        Fake f; Cache c(DEVICE, true, FakeBackend{&f});
        void *a = c.alloc(1000), *b = c.alloc(200 * MiB), *live = c.alloc(5000);
        f.dev = 1;
        void *d = c.alloc(3000);
        c.free(a); c.free(b); c.free(d);
        EXPECT(c.idle_blocks() == 3 && c.live_blocks() == 1 && f.releases == 0, "idle %zu", c.idle_blocks());
        f.fail_next = 1;
        void *p = c.alloc(70000);
        EXPECT(p && f.fail_next == 0 && f.releases == 3 && c.idle_blocks() == 0 && c.idle_classed_bytes() == 0 && c.idle_exact_bytes() == 0, "releases %ld", f.releases);
        EXPECT(c.live_blocks() == 2 && f.asked.size() == 6 && f.asked[4] == f.asked[5], "live %zu", c.live_blocks());
        // refused twice: nothing, and nothing recorded
        c.free(p);
        f.fail_next = 2;
        EXPECT(c.alloc(90000) == nullptr && f.fail_next == 0 && c.live_blocks() == 1 && c.idle_blocks() == 0 && f.releases == 4, "live %zu", c.live_blocks());
        EXPECT(c.alloc(300 * MiB) != nullptr && c.live_blocks() == 2, "no block after the refusals");
        (void)live;
    }
    {   // a pointer the cache never handed out goes to the backend
        Fake f; Cache c(DEVICE, true, FakeBackend{&f});
        void *x = f.make();
        EXPECT(c.free(x) == TRC_POOL_RELEASED && f.releases == 1 && f.foreign == 0 && f.out.empty() && f.quiesces == 0, "releases %ld", f.releases);
    }
}

static void check_host_policy() {
    Fake f; Cache c(HOST, true, FakeBackend{&f});
    void *p = c.alloc(300 * MiB + 1);
    EXPECT(f.asked.back() == trc_pool_class(300 * MiB + 1) && f.asked.back() == 320 * MiB, "asked %zu", f.asked.back());
    EXPECT(c.free(p) == TRC_POOL_KEPT && c.alloc(300 * MiB + 5) == p && f.allocs == 1, "allocs %ld", f.allocs);
    int local = 0;
    EXPECT(c.free(&local) == TRC_POOL_UNKNOWN && f.releases == 0 && f.foreign == 0, "a foreign pointer went to the backend");
    // every size is classed, and 4 GiB wait at most
    void *a = c.alloc(3 * GiB), *b = c.alloc(2 * GiB - 5);
    EXPECT(c.free(a) == TRC_POOL_KEPT && c.free(b) == TRC_POOL_RELEASED && c.free(p) == TRC_POOL_KEPT, "the 4 GiB cap");
    EXPECT(c.idle_classed_bytes() == 3 * GiB + 320 * MiB && c.idle_exact_bytes() == 0, "idle %zu", c.idle_classed_bytes());
    f.fail_next = 1;
    EXPECT(c.alloc(0) != nullptr && f.asked.back() == 256 && c.idle_blocks() == 0, "asked %zu", f.asked.back());
    EXPECT(f.quiesces == 0, "quiesces %ld", f.quiesces);
}

static void check_off() {
    Fake f; Cache c(DEVICE, false, FakeBackend{&f});
    for (size_t bytes : {(size_t)1, (size_t)1000, 128 * MiB + 3, 200 * MiB + 3, 3 * GiB}) {
        void *p = c.alloc(bytes);
        EXPECT(p && f.asked.back() == bytes, "asked %zu for %zu", f.asked.back(), bytes);
        EXPECT(c.idle_blocks() == 0 && c.free(p) == TRC_POOL_RELEASED && c.idle_blocks() == 0 && c.idle_classed_bytes() + c.idle_exact_bytes() == 0, "kept a block of %zu", bytes);
    }
    EXPECT(f.allocs == 5 && f.releases == 5 && f.quiesces == 0 && f.foreign == 0 && f.out.empty() && c.live_blocks() == 0, "allocs %ld releases %ld", f.allocs, f.releases);
    f.fail_next = 1;
    EXPECT(c.alloc(1000) == nullptr && f.asked.size() == 6, "off: a refused allocation was made again");
}

// eight threads on one cache under a scaled-down policy, then the books
static void check_accounting() {
    const trc_pool_policy small = {4 * KiB, 64 * KiB, 32 * KiB, true, true};
    Fake f; Cache c(small, true, FakeBackend{&f});
    std::atomic<long> nulls(0);
    auto worker = [&](unsigned seed) {
        std::mt19937 rng(seed);
        std::vector<void *> held;
        const size_t exact_sizes[] = {5000, 5001, 9000, 20000, 40000};      // (the last is never kept)
        for (int op = 0; op < 20000; ++op) {
            const unsigned r = rng();
            if (r % 997 == 0) f.fail_next += 1 + (r >> 10) % 2;
            if (r % 211 == 0) f.dev = (r >> 12) % 2;
            if (held.size() < 16 && (held.empty() || (r >> 4) % 2)) {
                const size_t bytes = (r >> 5) % 10 < 7 ? 1 + (r >> 9) % (4 * KiB) : exact_sizes[(r >> 9) % 5];
                void *p = c.alloc(bytes);
                if (p) held.push_back(p); else ++nulls;
            } else {
                const size_t i = (r >> 5) % held.size();
                EXPECT(c.free(held[i]) != TRC_POOL_UNKNOWN, "a block of the cache's was not known to it");
                held[i] = held.back(); held.pop_back();
            }
            if (op % 64 == 0) EXPECT(c.idle_classed_bytes() <= small.keep_classed && c.idle_exact_bytes() <= small.keep_exact, "more idle than the caps allow");
        }
        for (void *p : held) c.free(p);
    };
    std::vector<std::thread> ts;
    for (unsigned t = 0; t < 8; ++t) ts.emplace_back(worker, 1000 + t);
    for (std::thread &t : ts) t.join();
    c.trim();
    EXPECT(f.out.empty(), "%zu blocks outstanding", f.out.size());
    EXPECT(f.allocs == f.releases && f.foreign == 0, "allocs %ld releases %ld, %ld not the backend's", f.allocs, f.releases, f.foreign);
    EXPECT(c.live_blocks() == 0 && c.idle_blocks() == 0 && c.idle_classed_bytes() == 0 && c.idle_exact_bytes() == 0, "live %zu idle %zu", c.live_blocks(), c.idle_blocks());
    std::printf("accounting: %ld blocks from the backend, %ld kept at least once, %ld requests refused\n", f.allocs, f.quiesces, nulls.load());
}

int main() {
    check_classes();
    check_device_policy();
    check_host_policy();
    check_off();
    check_accounting();
    std::printf("pool_check: %d violations\n", bad.load());
    return bad > 255 ? 255 : bad.load();
}
