// entities_edit.hip -- the verbs that rewrite or hand over entity rows outside an update: a frame's touched inputs in,
// new tenants placed into a standing layout, rebuilt or selected rows out to a host mirror.
#include "common.h"
#include "entities_row.h"

namespace clapgpu {

// ---- a host mirror's small frames: touched inputs in, rebuilt outputs out, through device-mapped host memory -----------
// A frame of a testbed-sized scene (BASELINE configs[0]: 10 k entities) is a 15-30 us kernel; staged through device
// slabs it paid three copies' fixed latencies and a blocking wait on top (0.15 ms).  Letting the update kernel itself
// work on mapped host memory removes the copies but puts a PCIe round trip under every dependent load of its row walk
// (measured: 27 -> 54 us).  So the update kernel stays on device memory, untouched, between two small streaming kernels:
//   k_entities_apply_inputs   reads the frame's touched (slot, flags, TRS) records from mapped host memory -- one
//                             coalesced 40-byte stream -- and scatters them into the device arrays;
//   k_entities_export_rebuilt copies what the update rebuilt (its own rebuilt_mask says which slots) and the three bit
//                             masks into the host's result arrays, then raises a completion word the host polls.
__global__ __launch_bounds__(ENT_BLOCK)
void k_entities_apply_inputs(float4 *pos_scale, float4 *rot, uint32_t *flags, const clapgpu_entity_input *list,
                             uint32_t n_list, uint32_t n)
{
    const uint32_t k = blockIdx.x * ENT_BLOCK + threadIdx.x;
    if (k >= n_list) return;
    const uint32_t *r = reinterpret_cast<const uint32_t *>(list + k);     // 40-byte records: ten dwords, 8-byte aligned
    const uint2 h = *reinterpret_cast<const uint2 *>(r);
    const uint32_t slot = h.x;
    if (slot >= n) return;
    const uint2 a = *reinterpret_cast<const uint2 *>(r + 2), b = *reinterpret_cast<const uint2 *>(r + 4);
    const uint2 c = *reinterpret_cast<const uint2 *>(r + 6), d = *reinterpret_cast<const uint2 *>(r + 8);
    pos_scale[slot] = make_float4(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(b.x), __uint_as_float(b.y));
    rot[slot] = make_float4(__uint_as_float(c.x), __uint_as_float(c.y), __uint_as_float(d.x), __uint_as_float(d.y));
    flags[slot] = h.y;
}

// The lanes of a standing layout that got a new tenant between two frames (clapgpu_entities_place): 16-byte records.
__global__ __launch_bounds__(WAVE)
void k_entities_place(int32_t *parent, int32_t *model, float *aabb, float *center, const clapgpu_entity_place *list, uint32_t n_list,
                      uint32_t n, unsigned long long *stale)
{
    const uint32_t k = blockIdx.x * WAVE + threadIdx.x;
    if (k >= n_list) return;
    const uint4 r = *reinterpret_cast<const uint4 *>(list + k);
    const uint32_t slot = r.x;
    if (slot >= n) return;
    parent[slot] = (int32_t)r.y;
    model[slot] = (int32_t)r.z;
    if ((r.w & CLAPGPU_PLACE_CLEAR_STALE) && stale)
        atomicAnd(&stale[slot >> 6], ~(1ull << (slot & 63)));
    if (r.w & CLAPGPU_PLACE_ZERO_BOX) {
        float2 *b = reinterpret_cast<float2 *>(aabb + 6 * (size_t)slot);
        b[0] = b[1] = b[2] = make_float2(0.f, 0.f);
        float *c = center + 3 * (size_t)slot;
        c[0] = c[1] = c[2] = 0.f;
    }
}

struct ExportK {
    const float *mx, *inv_mx, *aabb, *center;            // device (the update's outputs)
    const uint64_t *vis_mask, *rebuilt_mask, *inside_mask;
    const uint64_t *select;                              // clapgpu_entities_export_rows: these rows, and no masks
    uint64_t *stale;                                     // ... whose stale bits (clapgpu_entities_hostio.stale_mask) are cleared
    float *o_mx, *o_inv, *o_aabb, *o_center;             // device-mapped host memory
    uint64_t *o_vis, *o_rebuilt, *o_inside;
    uint32_t *counter, *done, done_value, n_rows;
};

__global__ __launch_bounds__(ENT_BLOCK)
void k_entities_export_rebuilt(ExportK x)
{
    const int lane = lane_id();
    const uint32_t row = blockIdx.x * (ENT_BLOCK / WAVE) + threadIdx.x / WAVE;
    if (row < x.n_rows) {
        const uint64_t m = x.select ? x.select[row] : x.rebuilt_mask[row];
        if (lane == 0 && x.select && x.stale && m) x.stale[row] &= ~m;
        if (lane == 0 && !x.select) {
            x.o_rebuilt[row] = m;
            if (x.vis_mask) x.o_vis[row] = x.vis_mask[row];
            if (x.o_inside) x.o_inside[row] = x.inside_mask ? x.inside_mask[row] : 0ull;
        }
        if ((m >> lane) & 1ull) {
            const size_t i = (size_t)row * WAVE + lane;
            const float4 *a = reinterpret_cast<const float4 *>(x.mx + 16 * i), *b = reinterpret_cast<const float4 *>(x.inv_mx + 16 * i);
            float4 *oa = reinterpret_cast<float4 *>(x.o_mx + 16 * i), *ob = reinterpret_cast<float4 *>(x.o_inv + 16 * i);
            const float4 a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
            const float2 *bb = reinterpret_cast<const float2 *>(x.aabb + 6 * i);
            const float2 c0 = bb[0], c1 = bb[1], c2 = bb[2];
            const float *ct = x.center + 3 * i;
            const float t0 = ct[0], t1 = ct[1], t2 = ct[2];
            oa[0] = a0; oa[1] = a1; oa[2] = a2; oa[3] = a3;
            ob[0] = b0; ob[1] = b1; ob[2] = b2; ob[3] = b3;
            float2 *obb = reinterpret_cast<float2 *>(x.o_aabb + 6 * i);
            obb[0] = c0; obb[1] = c1; obb[2] = c2;
            float *oc = x.o_center + 3 * i;
            oc[0] = t0; oc[1] = t1; oc[2] = t2;
        }
    }
    raise_done_when_last(x.counter, x.done, x.done_value);
}

} // namespace clapgpu

using namespace clapgpu;

extern "C" int clapgpu_entities_apply_inputs(void *stream, const clapgpu_entities *e, const clapgpu_entity_input *list,
                                             uint32_t n_list)
{
    static_assert(sizeof(clapgpu_entity_input) == 40, "record layout");
    if (!e || !e->pos_scale || !e->rot || !e->flags || (n_list && !list))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (!n_list || !e->n)
        return CLAPGPU_OK;
    hipLaunchKernelGGL(k_entities_apply_inputs, dim3((n_list + ENT_BLOCK - 1) / ENT_BLOCK), dim3(ENT_BLOCK), 0, as_stream(stream),
                       reinterpret_cast<float4 *>(const_cast<float *>(e->pos_scale)),
                       reinterpret_cast<float4 *>(const_cast<float *>(e->rot)), e->flags, list, n_list, e->n);
    CLAPGPU_LAUNCH_CHECK("k_entities_apply_inputs");
    return CLAPGPU_OK;
}

extern "C" int clapgpu_entities_place(void *stream, const clapgpu_entities *e, const clapgpu_entity_place *list, uint32_t n_list,
                                      uint64_t *stale_mask)
{
    if (!e || !e->parent || !e->model || !e->aabb || !e->center || (n_list && !list))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (!n_list || !e->n)
        return CLAPGPU_OK;
    hipLaunchKernelGGL(k_entities_place, dim3((n_list + WAVE - 1) / WAVE), dim3(WAVE), 0, as_stream(stream),
                       const_cast<int32_t *>(e->parent), const_cast<int32_t *>(e->model), e->aabb, e->center, list, n_list, e->n,
                       reinterpret_cast<unsigned long long *>(stale_mask));
    CLAPGPU_LAUNCH_CHECK("k_entities_place");
    return CLAPGPU_OK;
}

// Both export verbs: the update's outputs to the mirror's arrays, and the completion word.  They differ in which rows
// go -- `select` (then with `stale`, whose bits of those rows are cleared, and no masks) or, with select == NULL, the rows
// of the update's own rebuilt_mask, with the three masks.
static int launch_export(void *stream, const clapgpu_entities *e, const clapgpu_entities_export *x, const uint64_t *select,
                         const char *what)
{
    ExportK k = {};
    k.mx = e->mx; k.inv_mx = e->inv_mx; k.aabb = e->aabb; k.center = e->center;
    k.o_mx = x->mx; k.o_inv = x->inv_mx; k.o_aabb = x->aabb; k.o_center = x->center;
    k.counter = x->counter; k.done = x->done; k.done_value = x->done_value; k.n_rows = e->n / 64;
    if (select) {
        k.select = select; k.stale = x->stale_mask;
    } else {
        k.vis_mask = e->vis_mask; k.rebuilt_mask = e->rebuilt_mask;
        k.inside_mask = (e->bv && e->bv->inside_mask) ? e->bv->inside_mask : nullptr;
        k.o_vis = x->vis_mask; k.o_rebuilt = x->rebuilt_mask; k.o_inside = x->inside_mask;
    }
    const uint32_t per_block = ENT_BLOCK / WAVE;
    const uint32_t blocks = k.n_rows ? (k.n_rows + per_block - 1) / per_block : 1;
    hipLaunchKernelGGL(k_entities_export_rebuilt, dim3(blocks), dim3(ENT_BLOCK), 0, as_stream(stream), k);
    CLAPGPU_LAUNCH_CHECK(what);
    return CLAPGPU_OK;
}

extern "C" int clapgpu_entities_export_rebuilt(void *stream, const clapgpu_entities *e, const clapgpu_entities_export *x)
{
    if (!e || !x || !e->mx || !e->inv_mx || !e->aabb || !e->center || !e->rebuilt_mask || !x->mx || !x->inv_mx || !x->aabb ||
        !x->center || !x->rebuilt_mask || !x->counter || !x->done || (e->vis_mask && !x->vis_mask))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (e->n & 63u)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    return launch_export(stream, e, x, nullptr, "k_entities_export_rebuilt");
}

extern "C" int clapgpu_entities_export_rows(void *stream, const clapgpu_entities *e, const clapgpu_entities_export *x,
                                            const uint64_t *select_mask)
{
    if (!e || !x || !select_mask || !e->mx || !e->inv_mx || !e->aabb || !e->center || !x->mx || !x->inv_mx || !x->aabb ||
        !x->center || !x->counter || !x->done)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (e->n & 63u)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    return launch_export(stream, e, x, select_mask, "k_entities_export_rows");
}
