// The caching layer under dev_alloc / DevBuf (ctx.h): freed device blocks of 64 MB and more stay mapped and are handed out again.
// No kernel is launched here.
#include <mutex>
#include <unordered_map>
#include <vector>

#include "ctx.h"

namespace {
struct DevBlock { void *p; size_t bytes; int device; };
std::mutex g_cache_mu;
std::vector<DevBlock> g_cache_free;                 // freed, still mapped
std::unordered_map<void *, DevBlock> g_cache_live;  // handed out by dev_cache_malloc
const size_t CACHE_MIN = 64ull << 20;               // smaller blocks go straight to the driver
}  // namespace

hipError_t dev_cache_malloc(void **p, size_t bytes)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (bytes >= CACHE_MIN) {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        size_t best = (size_t)-1;
        for (size_t i = 0; i < g_cache_free.size(); i++) {
            const DevBlock &b = g_cache_free[i];
            // fits, is at most twice the request, and is the tightest such block
            if (b.device == dev && b.bytes >= bytes && b.bytes - bytes <= bytes &&
                (best == (size_t)-1 || b.bytes < g_cache_free[best].bytes))
                best = i;
        }
        if (best != (size_t)-1) {
            DevBlock b = g_cache_free[best];
            g_cache_free.erase(g_cache_free.begin() + (long)best);
            g_cache_live[b.p] = b;
            *p = b.p;
            return hipSuccess;
        }
    }
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {  // out of memory: give the cached blocks back and try once more
        (void)hipGetLastError();
        dev_cache_trim();
        e = hipMalloc(p, bytes);
    }
    if (e == hipSuccess && bytes >= CACHE_MIN) {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        g_cache_live[*p] = DevBlock{*p, bytes, dev};
    }
    return e;
}

void dev_cache_free(void *p)
{
    if (!p) return;
    DevBlock blk{};
    bool cached = false;
    {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        auto it = g_cache_live.find(p);
        if (it != g_cache_live.end()) {
            blk = it->second;
            g_cache_live.erase(it);
            cached = true;
        }
    }
    if (!cached) {
        (void)hipFree(p);
        return;
    }
    // hipFree would have waited for the block's device; a block handed out again must not still be in use either.  The wait is
    // for the BLOCK's device (a shard thread may free another shard's block) and happens outside the lock: other shards'
    // allocations do not queue behind it.
    int cur = 0;
    (void)hipGetDevice(&cur);
    if (cur != blk.device) (void)hipSetDevice(blk.device);
    (void)hipDeviceSynchronize();
    if (cur != blk.device) (void)hipSetDevice(cur);
    std::lock_guard<std::mutex> lk(g_cache_mu);
    g_cache_free.push_back(blk);
}

// a block nobody has used yet goes to the free list as it is (no device synchronisation needed)
void dev_cache_park(void *p, size_t bytes, int device)
{
    std::lock_guard<std::mutex> lk(g_cache_mu);
    g_cache_free.push_back(DevBlock{p, bytes, device});
}

void dev_cache_trim(int device)
{
    std::vector<DevBlock> blocks;
    {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        if (device < 0) blocks.swap(g_cache_free);
        else {  // only this device's blocks: the other shards of a multi-device ctx may still be building from theirs
            std::vector<DevBlock> keep;
            for (const DevBlock &b : g_cache_free) (b.device == device ? blocks : keep).push_back(b);
            g_cache_free.swap(keep);
        }
    }
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (const DevBlock &b : blocks) {
        (void)hipSetDevice(b.device);
        (void)hipFree(b.p);
    }
    (void)hipSetDevice(cur);
}
