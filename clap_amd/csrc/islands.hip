// islands.hip -- the island pass of dWorldQuickStep for gfx950: a sleeping body that touches an awake one wakes.
//
// phys_body_new puts every dynamic body on auto-disable and relies on ODE to bring it back: "ODE re-enables them
// automatically when another enabled body collides with them" (physics.c:1034-1042).  That happens in dxProcessIslands
// (ODE 0.16 util.cpp, restated; ODE is absent from the reference: PARITY UNPINNED), which dWorldQuickStep (physics.c:769)
// runs in this order: dInternalHandleAutoDisabling; islands grown from every body still enabled along the joints between
// two bodies, every body reached losing dxBodyDisabled and nothing else ("Body disabled flag is not checked here.  This is
// how auto-enable works."); the step of the enabled bodies.  Connected components, no solver.
//   k_islands_seed     one lane per body: the auto-disable bookkeeping the step would do (adis_dev.h), then
//                      HAS_JOINT cleared on every body (dJointGroupEmpty moved forward: the step that follows skips its
//                      own bookkeeping and integrates), parent[i] = i, awake[i] = 0
//   k_islands_link     one lane per touching body-body pair: union-find over parent[], the larger root hooked under the
//                      smaller by compare-and-swap, so that a component's root is its smallest index
//   k_islands_resolve  one lane per body: its root (the island), and an enabled body marks its root awake
//   k_islands_wake     one lane per body: a DISABLED body whose root is marked loses the flag; the count
// What one launch leaves for the next crosses a kernel boundary.  INSIDE the link launch lanes on different CUs and XCDs
// work on the same words, a CU's L1 is never refreshed by another CU's stores and the XCDs' L2s are not coherent, so every
// access to a parent word, in every launch, is an agent-scope relaxed atomic on a non-const pointer (no plain load, no
// scalar-cache path).  The union does not need such a load to be fresh: parent[x] only ever decreases, and every value
// it has held is an ancestor of x in the final forest, so a load that returns an older value walks a longer way to the
// same tree; the one operation that has to see the present is the hook's compare-and-swap, and it is made where atomics
// are made.  No fences, no flags, no lane waits for another.
#include "common.h"
#include "adis_dev.h"

namespace clapgpu {

constexpr int IB = 256;
constexpr int WB = 1024;                                // k_islands_wake
constexpr uint32_t LINK_BLOCKS_MAX = 2048;              // the link launch strides over the pairs

struct IslandsK {
    uint32_t n, samples;
    double *lvel, *avel;
    uint32_t *bflags;
    int32_t *adis_steps_left;
    double *adis_time_left;
    double *adis_samples;
    uint32_t *adis_counter;
};

__device__ __forceinline__ uint32_t parent_load(uint32_t *parent, uint32_t x)
{
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x as this lane can see it: parent values only decrease, so the walk ends after at most x loads.  With
// HALVE every node on the way is pointed at its grandparent (atomic min: the word still only decreases, and the new
// value is an ancestor); it keeps the trees of a long chain shallow and asks for no retry.
template <bool HALVE>
__device__ __forceinline__ uint32_t find_root(uint32_t *parent, uint32_t x)
{
    uint32_t p = parent_load(parent, x);
    while (p != x) {
        const uint32_t g = parent_load(parent, p);
        if (HALVE && g != p)
            (void)__hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = g;
    }
    return x;
}

__global__ __launch_bounds__(IB)
void k_islands_seed(IslandsK b, clapgpu_world w, double h, uint32_t *parent, uint32_t *awake, uint32_t *woken_total)
{
    const uint32_t i = blockIdx.x * IB + threadIdx.x;
    if (i == 0 && woken_total) *woken_total = 0;
    if (i >= b.n) return;
    __hip_atomic_store(parent + i, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    awake[i] = 0;
    const uint32_t fl = b.bflags[i];
    if (!(fl & CLAPGPU_BODY_HAS_JOINT)) return;                             // nothing to book, nothing to clear
    if (!(fl & CLAPGPU_BODY_DISABLED) && (fl & CLAPGPU_BODY_AUTO_DISABLE)) {
        const double *vp = b.lvel + 3 * (size_t)i, *op = b.avel + 3 * (size_t)i;
        const double v[3] = { vp[0], vp[1], vp[2] }, om[3] = { op[0], op[1], op[2] };
        if (auto_disable(b, w, h, i, fl, v, om)) return;           // asleep, HAS_JOINT dropped with it
    }
    b.bflags[i] = fl & ~CLAPGPU_BODY_HAS_JOINT;                             // dJointGroupEmpty, ahead of the step
}

__global__ __launch_bounds__(IB)
void k_islands_link(uint32_t n, const uint2 *pairs, const uint32_t *pair_total, uint32_t capacity,
                    const clapgpu_contact2 *contacts, uint32_t *parent)
{
    const uint32_t total = *pair_total < capacity ? *pair_total : capacity;
    for (uint32_t k = blockIdx.x * IB + threadIdx.x; k < total; k += gridDim.x * IB) {
        if ((contacts[k].nc & ~CLAPGPU_CONTACT_DEEP) < 1) continue;
        const uint2 pr = pairs[k];
        if (pr.x >= n || pr.y >= n || pr.x == pr.y) continue;
        uint32_t a = pr.x, c = pr.y;
        for (;;) {
            a = find_root<true>(parent, a);
            c = find_root<true>(parent, c);
            if (a == c) break;                                              // one tree: they were joined, by whomever
            const uint32_t hi = a > c ? a : c, lo = a > c ? c : a;
            uint32_t seen = hi;
            if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT))
                break;
            // another lane's hook or halving won parent[hi]: `seen` is what it holds now, below hi and in hi's tree.
            // Going on from there, a + c falls with every retry, whatever the loads return: at most 2 n of them.
            a = seen;
            c = lo;
        }
    }
}

__global__ __launch_bounds__(IB)
void k_islands_resolve(uint32_t n, const uint32_t *bflags, uint32_t *parent, uint32_t *awake, uint32_t *root)
{
    const uint32_t i = blockIdx.x * IB + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = find_root<false>(parent, i);                         // nobody writes parent[] in this launch
    root[i] = r;
    if (!(bflags[i] & CLAPGPU_BODY_DISABLED))
        __hip_atomic_store(awake + r, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // every writer writes 1
}

// the count: a ballot per wavefront into LDS, one atomic per workgroup of 16 wavefronts that woke somebody (one per
// wavefront was 4 096 atomics on one word at 262 144 bodies, and most of the launch)
__global__ __launch_bounds__(WB)
void k_islands_wake(uint32_t n, uint32_t *bflags, const uint32_t *awake, const uint32_t *root, uint32_t *woken_total)
{
    __shared__ uint32_t count;
    if (threadIdx.x == 0) count = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * WB + threadIdx.x;
    bool wakes = false;
    if (i < n) {
        const uint32_t fl = bflags[i];
        wakes = (fl & CLAPGPU_BODY_DISABLED) && awake[root[i]];
        if (wakes) bflags[i] = fl & ~CLAPGPU_BODY_DISABLED;                 // dxBodyDisabled alone: the counters stay spent
    }
    if (!woken_total) return;                                               // the same for every lane of the launch
    const unsigned long long m = __ballot(wakes);
    if (m && lane_id() == __ffsll(m) - 1) atomicAdd(&count, (uint32_t)__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0 && count) atomicAdd(woken_total, count);
}

// the scratch: parent [n] | awake [n] | root [n] (the last unused when the caller takes `island`)
struct IslandsLayout { size_t parent, awake, root, total; };

static IslandsLayout islands_layout(uint32_t n)
{
    IslandsLayout l;
    Carve c;
    l.parent = c.take((size_t)n * sizeof(uint32_t));
    l.awake = c.take((size_t)n * sizeof(uint32_t));
    l.root = c.take((size_t)n * sizeof(uint32_t));
    l.total = c.bytes();
    return l;
}

} // namespace clapgpu

using namespace clapgpu;

extern "C" size_t clapgpu_bodies_islands_scratch_bytes(uint32_t n)
{
    return islands_layout(n).total;
}

extern "C" int clapgpu_bodies_islands(void *stream, const clapgpu_bodies *b, const clapgpu_world *w, double h,
                                      const uint32_t *pairs, const uint32_t *pair_total, uint32_t capacity,
                                      const clapgpu_contact2 *contacts, void *scratch, uint32_t *island, uint32_t *woken_total)
{
    int rc = check_bodies(b);
    if (rc) return rc;
    if (!w || !pair_total || (capacity && (!pairs || !contacts))) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if ((reinterpret_cast<uintptr_t>(pairs) & 7u) || (reinterpret_cast<uintptr_t>(contacts) & 15u) ||
        (reinterpret_cast<uintptr_t>(pair_total) & 3u) || (reinterpret_cast<uintptr_t>(island) & 3u) ||
        (reinterpret_cast<uintptr_t>(woken_total) & 3u))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    const uint32_t n = b->n;
    if (n == 0) return CLAPGPU_OK;
    if (!scratch || (reinterpret_cast<uintptr_t>(scratch) & 255u)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    hipStream_t s = as_stream(stream);
    const IslandsLayout l = islands_layout(n);
    uint8_t *base = static_cast<uint8_t *>(scratch);
    uint32_t *parent = reinterpret_cast<uint32_t *>(base + l.parent), *awake = reinterpret_cast<uint32_t *>(base + l.awake);
    uint32_t *root = island ? island : reinterpret_cast<uint32_t *>(base + l.root);

    IslandsK k;
    k.n = n; k.samples = b->adis_average_samples;
    k.lvel = b->lvel; k.avel = b->avel; k.bflags = b->bflags;
    k.adis_steps_left = b->adis_steps_left; k.adis_time_left = b->adis_time_left;
    k.adis_samples = b->adis_samples; k.adis_counter = b->adis_counter;
    const dim3 grid((n + IB - 1) / IB);
    hipLaunchKernelGGL(k_islands_seed, grid, dim3(IB), 0, s, k, *w, h, parent, awake, woken_total);
    CLAPGPU_LAUNCH_CHECK("k_islands_seed");
    if (capacity) {
        const uint32_t blocks = (capacity + IB - 1) / IB;
        hipLaunchKernelGGL(k_islands_link, dim3(blocks < LINK_BLOCKS_MAX ? blocks : LINK_BLOCKS_MAX), dim3(IB), 0, s, n,
                           reinterpret_cast<const uint2 *>(pairs), pair_total, capacity, contacts, parent);
        CLAPGPU_LAUNCH_CHECK("k_islands_link");
    }
    hipLaunchKernelGGL(k_islands_resolve, grid, dim3(IB), 0, s, n, b->bflags, parent, awake, root);
    CLAPGPU_LAUNCH_CHECK("k_islands_resolve");
    hipLaunchKernelGGL(k_islands_wake, dim3((n + WB - 1) / WB), dim3(WB), 0, s, n, b->bflags, awake, root, woken_total);
    CLAPGPU_LAUNCH_CHECK("k_islands_wake");
    return CLAPGPU_OK;
}
