// trc_pool.h -- the block cache behind the library's device memory and its pinned host memory: the policy, with no device in it.
//
// A freed block is kept for the next request of its size instead of going back to the driver (mapping and releasing a block of a
// few MB costs ~0.3 ms each, and page-locking 250 MB takes longer than copying them).  Requests up to `class_max` bytes are
// rounded up to size classes an eighth of an octave apart (at most 12.5 % over the request) and at most `keep_classed` bytes of
// them wait idle.  Larger requests are "exact": they are not rounded -- the driver was seen to stall for 1.2 s on a *rounded* large
// size -- and a freed one waits for the next request of exactly its size (a Monte-Carlo loop asks for the same 0.9 GB level call
// after call); at most `keep_exact` bytes of them wait idle, and the oldest make room for a new one.  A request the backend
// refuses empties the cache and is made once more.
//
// The cache is templated on a backend, which is all it knows of a device:
//     void *alloc(size_t bytes)      a new block, or nullptr
//     void release(void *p)          a block of alloc() back to where it came from
//     void quiesce()                 returns when nothing in flight can still use a block freed before the call
//     int device()                   the device a block allocated now would belong to
// trc_host.h (device memory) and trc_scene.hip (pinned host memory) have the two real ones; tests/poolcheck drives the cache
// through a fake one under the sanitizers.  Nothing here includes a HIP header.
#ifndef TRC_POOL_H
#define TRC_POOL_H

#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>
#include <unordered_map>
#include <utility>
#include <vector>

// the size class of a request: the next multiple of an eighth of the power of two below it, 256 at the least
static inline size_t trc_pool_class(size_t bytes) {
    if (bytes <= 256) return 256;
    const int k = 63 - __builtin_clzll((unsigned long long)bytes);      // 2^k <= bytes
    const size_t step = (size_t)1 << (k - 3);
    return (bytes + step - 1) & ~(step - 1);
}

struct trc_pool_policy {
    size_t class_max;         // requests above it are exact: neither rounded nor classed
    size_t keep_classed;      // idle bytes of classed blocks, at most
    size_t keep_exact;        // idle bytes of exact blocks, at most, and the largest exact block ever kept
    bool release_unknown;     // free() of a pointer the cache did not hand out: release it to the backend, or report it
    bool quiesce_kept;        // a block that is kept waits for the backend's quiesce() first (memory that work in flight may still use)
};

enum trc_pool_freed { TRC_POOL_KEPT, TRC_POOL_RELEASED, TRC_POOL_UNKNOWN };

template <class Backend>
class trc_block_cache {
    typedef std::pair<int, size_t> Key;                    // (device, bytes asked of the backend)
    struct Idle { void *p; uint64_t seq; };
    typedef std::multimap<Key, Idle> IdleMap;

    const trc_pool_policy pol_;
    const bool on_;
    Backend be_;
    mutable std::mutex mu_;
    std::unordered_map<void *, Key> live_;                 // block handed out -> its key, as of the allocation
    IdleMap idle_;                                         // blocks waiting
    std::map<uint64_t, typename IdleMap::iterator> exact_order_;      // the exact ones among them, oldest first
    uint64_t seq_ = 0;
    size_t idle_classed_ = 0, idle_exact_ = 0;             // bytes waiting, and bytes of blocks on their way into idle_ (free())

    bool exact(size_t bytes) const { return bytes > pol_.class_max; }

    // an idle block out of the books (mu_ held)
    void *take(typename IdleMap::iterator it) {
        void *p = it->second.p;
        const size_t n = it->first.second;
        if (exact(n)) { idle_exact_ -= n; exact_order_.erase(it->second.seq); }
        else idle_classed_ -= n;
        idle_.erase(it);
        return p;
    }

public:
    trc_block_cache(const trc_pool_policy &pol, bool on, const Backend &be = Backend()) : pol_(pol), on_(on), be_(be) {}

    // a block of at least `bytes`, or nullptr when the backend has refused twice.  Off: the backend's, of `bytes` as given.
    void *alloc(size_t bytes) {
        if (!on_) return be_.alloc(bytes);
        const Key key(be_.device(), exact(bytes) ? bytes : trc_pool_class(bytes));
        {
            std::lock_guard<std::mutex> g(mu_);
            typename IdleMap::iterator it = idle_.find(key);
            if (it != idle_.end()) {
                void *p = take(it);
                live_[p] = key;
                return p;
            }
        }
        void *p = be_.alloc(key.second);
        if (!p) {
            trim();
            p = be_.alloc(key.second);
            if (!p) return nullptr;
        }
        std::lock_guard<std::mutex> g(mu_);
        live_[p] = key;
        return p;
    }

    // A block of alloc() back: kept under the key it was allocated with while the caps allow, released otherwise.  Where the policy
    // asks for it, a block that is kept gets one quiesce() before the next owner can have it; one that is released gets none, the
    // backend's release waits itself.
    trc_pool_freed free(void *p) {
        Key key(0, 0);
        bool keep = false;
        std::vector<void *> evict;
        if (on_) {
            std::lock_guard<std::mutex> g(mu_);
            typename std::unordered_map<void *, Key>::iterator it = live_.find(p);
            if (it != live_.end()) {
                key = it->second;
                live_.erase(it);
                const size_t n = key.second;
                if (exact(n)) {
                    if (n <= pol_.keep_exact) {
                        while (idle_exact_ + n > pol_.keep_exact && !exact_order_.empty()) evict.push_back(take(exact_order_.begin()->second));
                        keep = idle_exact_ + n <= pol_.keep_exact;
                    }
                } else keep = idle_classed_ + n <= pol_.keep_classed;
                if (keep) (exact(n) ? idle_exact_ : idle_classed_) += n;
            } else if (!pol_.release_unknown) return TRC_POOL_UNKNOWN;
        }
        if (keep) {
            if (pol_.quiesce_kept) be_.quiesce();
            std::lock_guard<std::mutex> g(mu_);
            typename IdleMap::iterator it = idle_.insert(std::make_pair(key, Idle{p, seq_}));
            if (exact(key.second)) exact_order_[seq_] = it;
            ++seq_;
        } else be_.release(p);
        for (void *q : evict) be_.release(q);
        return keep ? TRC_POOL_KEPT : TRC_POOL_RELEASED;
    }

    // every idle block of every device back to the backend
    void trim() {
        std::vector<void *> gone;
        {
            std::lock_guard<std::mutex> g(mu_);
            while (!idle_.empty()) gone.push_back(take(idle_.begin()));
        }
        for (void *p : gone) be_.release(p);
    }

    // what the books say, for tests
    size_t idle_blocks() const { std::lock_guard<std::mutex> g(mu_); return idle_.size(); }
    size_t idle_blocks(int device, size_t bytes) const { std::lock_guard<std::mutex> g(mu_); return idle_.count(Key(device, bytes)); }
    size_t idle_classed_bytes() const { std::lock_guard<std::mutex> g(mu_); return idle_classed_; }
    size_t idle_exact_bytes() const { std::lock_guard<std::mutex> g(mu_); return idle_exact_; }
    size_t live_blocks() const { std::lock_guard<std::mutex> g(mu_); return live_.size(); }
};

#endif
