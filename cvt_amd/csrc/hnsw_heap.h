// hnsw_heap.h -- the two priority queues of the reference's HNSW traversals, restated on arrays: libstdc++'s push_heap /
// pop_heap (__push_heap, __adjust_heap) with wave-wide reads, and the LDS / LDS + HBM array views they run on.  Shared by the
// search (hnsw.hip) and the construction (hnsw_build.hip): ties between equal distances fall as the reference's
// std::priority_queue lets them fall.
#ifndef CVTMI_HNSW_HEAP_H
#define CVTMI_HNSW_HEAP_H
#include "common.h"

namespace cvtmi {

constexpr int HN_EF_MAX = 1024;  // top queue: ef + 1 entries in LDS
constexpr int HN_LCAP = 256;    // candidate queue entries kept in LDS; the rest lives in HBM

struct HnEnt { float d; uint32_t id; };

// max-heap on d over an array addressed through A (get / set), n entries
template <class A>
__device__ __forceinline__ void hn_push_heap(A &a, int hole, HnEnt v)
{
    int parent = (hole - 1) / 2;
    while (hole > 0) {
        const HnEnt p = a.get(parent);
        if (!(p.d < v.d)) break;
        a.set(hole, p);
        hole = parent;
        parent = (hole - 1) / 2;
    }
    a.set(hole, v);
}
// The same sift-up with the whole ancestor chain taken at once: lane i reads ancestor i of the hole (the chain is known before
// anything is compared: positions (hole + 1) >> (i + 1), 1-based), one ballot finds the first ancestor that stays, the ancestors
// below it move down one step each and v lands above them -- two memory round trips whatever the depth, instead of one per level.
// Same comparisons, same final layout as __push_heap.
template <class A>
__device__ __forceinline__ void hn_push_heap_wave(A &a, int hole, HnEnt v, int lane)
{
    const int h1 = hole + 1;
    const int anc1 = lane < 31 ? (h1 >> (lane + 1)) : 0;      // 1-based ancestor i, 0 = past the root
    const bool valid = anc1 >= 1;
    HnEnt p; p.d = 0.0f; p.id = 0u;
    if (valid) p = a.get_l(anc1 - 1);
    const unsigned long long up = __ballot(valid && p.d < v.d);   // ancestor i is passed
    const int s_ = __ffsll((long long)~up) - 1;                    // first ancestor that stays (or the first lane past the root)
    const int below = lane == 0 ? hole : (h1 >> lane) - 1;         // the position one step below ancestor `lane` on the chain
    if (lane < s_) a.set_l(below, p);
    else if (lane == s_) a.set_l(below, v);
}
template <class A>
__device__ __forceinline__ void hn_push(A &a, int &n, float d, uint32_t id, int lane)
{
    HnEnt v; v.d = d; v.id = id;
    hn_push_heap_wave(a, n, v, lane);
    ++n;
}
// __adjust_heap walks from the root to a leaf, one comparison of two children per level: a chain of dependent reads, eleven deep for a
// queue of 2000 entries, the lower three or four of them in HBM.  Here the wave fetches the next FIVE levels below the hole at once --
// level j of that subtree is the 2^j consecutive entries from (hole + 1) 2^j - 1, lanes 2^j - 2 .. 2^(j+1) - 3 take it -- and the five
// comparisons run on register values (v_readlane with a uniform lane number): one memory round trip per five levels, same
// comparisons, same moves, same final layout.
__device__ __forceinline__ HnEnt hn_lane(const HnEnt &e, int src)
{
    HnEnt r;
    r.d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e.d), src));
    r.id = (uint32_t)__builtin_amdgcn_readlane((int)e.id, src);
    return r;
}
template <class A>
__device__ __forceinline__ void hn_pop(A &a, int &n, int lane)
{
    if (n > 1) {
        const int len = n - 1;
        int hole = 0, second = 0;
        const int limit = (len - 1) / 2;
        const int j = 31 - __clz(lane + 2);          // level of this lane's entry in the subtree (1 .. 5; lanes 62, 63 idle)
        const int off = lane + 2 - (1 << j);
        HnEnt value; value.d = 0.0f; value.id = 0u;
        bool have_value = false;
        while (second < limit) {
            const int pos = ((second + 1) << j) - 1 + off;
            HnEnt e; e.d = 0.0f; e.id = 0u;
            if (j <= 5 && pos < len) e = a.get_l(pos);
            if (!have_value) {                         // the entry that leaves the end of the array rides along with the first fetch (lane 63)
                if (lane == 63) e = a.get_l(len);
                value = hn_lane(e, 63);
                have_value = true;
            }
            int rel = 0;                               // offset of the hole within its level of the subtree
#pragma unroll
            for (int t = 0; t < 5; ++t) {
                if (second >= limit) break;
                second = 2 * (second + 1);
                const int lr = __builtin_amdgcn_readfirstlane((2 << t) - 2 + 2 * rel + 1);   // lane of the right child
                const HnEnt r = hn_lane(e, lr), l = hn_lane(e, lr - 1);
                HnEnt pick = r;
                rel = 2 * rel + 1;
                if (r.d < l.d) { --second; --rel; pick = l; }
                a.set(hole, pick);
                hole = second;
            }
        }
        if (!have_value) value = a.get(len);           // (len <= 2: no level to walk)
        if ((len & 1) == 0 && second == (len - 2) / 2) {
            second = 2 * (second + 1);
            a.set(hole, a.get(second - 1));
            hole = second - 1;
        }
        hn_push_heap_wave(a, hole, value, lane);
    }
    --n;
}

// Every lane runs the heap code with wave-uniform values; loads broadcast, lane 0 stores.
struct LdsArr {
    HnEnt *p; bool w;
    __device__ __forceinline__ HnEnt get(int i) const { return p[i]; }
    __device__ __forceinline__ void set(int i, HnEnt v) const { if (w) p[i] = v; }
    __device__ __forceinline__ HnEnt get_l(int i) const { return p[i]; }            // per-lane index
    __device__ __forceinline__ void set_l(int i, HnEnt v) const { p[i] = v; }
};
// first `cap` entries (the upper heap levels, touched by every operation) in LDS, the rest in HBM
struct SplitArr {
    HnEnt *l; HnEnt *g; bool w; int cap;
    __device__ __forceinline__ HnEnt get(int i) const { return i < cap ? l[i] : g[i - cap]; }
    __device__ __forceinline__ void set(int i, HnEnt v) const { if (w) { if (i < cap) l[i] = v; else g[i - cap] = v; } }
    __device__ __forceinline__ HnEnt get_l(int i) const { return i < cap ? l[i] : g[i - cap]; }   // per-lane index
    __device__ __forceinline__ void set_l(int i, HnEnt v) const { if (i < cap) l[i] = v; else g[i - cap] = v; }
};

}  // namespace cvtmi
#endif
