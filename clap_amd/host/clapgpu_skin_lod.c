/*
 * clapgpu_skin_lod.c -- the vertices each LOD of a model draws, from the engine's own index buffers: the lists
 * clapgpu_skin_drawn takes (see clapgpu_scene.h).  Host only; no device call.
 */
#include <stdlib.h>
#include <string.h>
#include "clapgpu_scene.h"

int clapgpu_skin_lod_lists(const uint16_t *const *index, const uint32_t *n_index, uint32_t n_lods, uint32_t n_verts,
                           uint32_t *list, uint32_t capacity, uint32_t *total, uint32_t *lod_first, uint32_t *lod_count)
{
    if (!index || !n_index || !total || !lod_first || !lod_count || n_lods < 1 || n_lods > CLAPGPU_SKIN_LODS || n_verts == 0 ||
        n_verts > 65536u || (capacity && !list))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    for (uint32_t l = 0; l < n_lods; l++) {
        if (n_index[l] && !index[l]) return CLAPGPU_ERR_INVALID_ARGUMENTS;
        for (uint32_t k = 0; k < n_index[l]; k++)
            if (index[l][k] >= n_verts) return CLAPGPU_ERR_OUT_OF_BOUNDS;
    }
    uint8_t *used = malloc(n_verts);
    if (!used) return CLAPGPU_ERR_NOMEM;
    uint64_t at = *total;
    for (uint32_t l = 0; l < n_lods; l++) {
        memset(used, 0, n_verts);
        uint32_t distinct = 0;
        for (uint32_t k = 0; k < n_index[l]; k++)
            if (!used[index[l][k]]) { used[index[l][k]] = 1; distinct++; }
        if (distinct == n_verts) {                          /* the whole mesh: no entries, no list read on the device */
            lod_first[l] = CLAPGPU_SKIN_LOD_ALL;
            lod_count[l] = n_verts;
            continue;
        }
        lod_first[l] = (uint32_t)(at < 0xffffffffu ? at : 0xfffffffeu);
        lod_count[l] = distinct;
        for (uint32_t v = 0; v < n_verts; v++) {            /* ascending, distinct */
            if (!used[v]) continue;
            if (at < capacity) list[at] = v;
            at++;
        }
    }
    free(used);
    *total = (uint32_t)(at < 0xffffffffu ? at : 0xffffffffu);
    return at > capacity ? CLAPGPU_ERR_TOO_LARGE : CLAPGPU_OK;
}
