// move_dev.h -- character_move's stages as move.hip issues them, for the two callers that run them: clapgpu_characters_move
// (all movers at once) and clapgpu_characters_move_ordered (order.hip: one contiguous slice of the movers per conflict
// level, the push once at the end).  Host only.
#pragma once
#include "common.h"

namespace clapgpu {

// the parts of clapgpu_characters_move's scratch (move.hip's move_layout), as pointers
struct MoveParts {
    uint32_t *words;                    // [b->n] the per-body words of the ray and the slide, one after the other
    uint32_t *slide_body, *slide_flags; // [n] the slide's list (0xffffffff: stands still) and its flags
    float *given;                       // [n][3] the velocity the push is given
    double *dist, *other;               // [n] the ray's distance and its mesh pass's word
    uint8_t *grounded, *grounded_out;   // [n]
    void *push;                         // clapgpu_bodies_push's own
};

// move.hip: the parts of a scratch of clapgpu_characters_move_scratch_bytes(n_bodies, n) bytes; CLAPGPU_ERR_TOO_LARGE /
// CLAPGPU_ERR_UNKNOWN when the push cannot size its part (as clapgpu_characters_move returns them)
__attribute__((visibility("hidden"))) int move_parts(void *scratch, uint32_t n_bodies, uint32_t n, MoveParts *p);

// move.hip: stages 1 to 5 of clapgpu_characters_move for the movers [at, at + count) of m, count > 0; the [n] parts of p
// are used at the same offset.  push: ... and clapgpu_bodies_push over that slice.  The arguments are checked already.
__attribute__((visibility("hidden"))) int move_slice(void *stream, clapgpu_bp *bp, const clapgpu_bodies *b, const clapgpu_world *w,
                                                     const clapgpu_geoms *statics, const clapgpu_trimesh *meshes, double dt_sec,
                                                     const clapgpu_move *m, uint32_t at, uint32_t count, const MoveParts &p,
                                                     bool push);

// move.hip: stage 6 and the flags (k_move_finish) for all m->n movers
__attribute__((visibility("hidden"))) int move_finish(void *stream, const clapgpu_entities *e, const clapgpu_move *m,
                                                      const MoveParts &p);

// move.hip: what clapgpu_characters_move refuses before any HIP call, but for the scratch
__attribute__((visibility("hidden"))) int move_check(clapgpu_bp *bp, const clapgpu_bodies *b, const clapgpu_world *w,
                                                     const clapgpu_geoms *statics, const clapgpu_entities *e, const clapgpu_move *m);

} // namespace clapgpu
