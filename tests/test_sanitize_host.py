"""The host C of the product under sanitizers, in a container without a GPU.

clap_amd/binding/gpu-scene.c (records, hash, tombstones, re-tiling, the worker pool, the write-back policies) and
clap_amd/host/clapgpu_scene*.c (handle table, tiler, upload image, stale / fetch bookkeeping) are the largest and most
pointer-heavy host C here; the reference's debug preset runs ASan + UBSan over ITS host code
(the reference's CMakeLists.txt:17-18, 33-39).  The drop-in checker (oracle/ref/dropin.c: the reference's own mq /
entity3d objects on both sides) is linked here against tests/c/fake_clapgpu.c -- a CPU stand-in for libclapgpu.so's
entry points, memory = malloc, the entity kernels = the oracle -- instead of the HIP library, and run under
-fsanitize=address,undefined and, separately, -fsanitize=thread with scenes large enough for the worker-thread passes.
TEST INFRASTRUCTURE: the fake is never shipped and proves nothing about the kernels (the -m gpu tests do that); what is
under test is the host code's memory and thread behaviour.  The checkers are compiled against the reference tree by
build() (oracle/ref/Makefile -> oracle/_ref/clap_dropin_{asan,tsan,plain}); they are absent wherever that tree was not.
"""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "c", "_build")
REF_OUT = os.path.join(ROOT, "oracle", "_ref")


def _build(kind):
    """The checker build() made: oracle/_ref/clap_dropin_<kind>."""
    exe = os.path.join(REF_OUT, f"clap_dropin_{kind}")
    if not os.access(exe, os.X_OK):
        pytest.skip(f"oracle/_ref/clap_dropin_{kind} not built (build() makes it where the reference tree is)")
    return exe


def _run(exe, *args, env=None, timeout=900):
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
             TSAN_OPTIONS="halt_on_error=0:second_deadlock_stack=1", **(env or {}))
    p = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=timeout, env=e)
    ours = [l for l in p.stderr.splitlines() if "runtime error:" in l and ("clap_amd/" in l or "tests/c/" in l or "oracle/" in l)]
    assert "AddressSanitizer" not in p.stderr and "ThreadSanitizer" not in p.stderr and not ours, p.stderr[-4000:]
    assert p.returncode == 0, f"{args}: rc {p.returncode}\n{p.stderr[-3000:]}"
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.timeout(1500)
def test_binding_and_mirror_under_asan_ubsan():
    """The scripted game (creations, deletions, re-parenting, host updates, hidden entities), both write-back policies,
    the LOD / draw-list passes, the hand-made edge scenes and the bench consumers: no invalid access, no leak of a freed
    record into a later frame, no undefined behaviour in our files -- and, since the fake computes with the oracle, still
    the reference's bits everywhere."""
    exe = _build("asan")
    assert _run(exe, "test", 2500, 12, 1, "notify", "drawn", "steady")["mismatches"] == 0
    # found by this very set-up: a stale entity deleted before the walk that would have fetched it (use after free), a
    # detached child whose parent_seq has to come from the parent it HAD, a host update of a stale entity's parent
    assert _run(exe, "test", 2000, 40, 7, "notify", "drawn", "steady")["mismatches"] == 0
    assert _run(exe, "test", 200, 40, 13, "notify", "drawn")["mismatches"] == 0
    assert _run(exe, "test", 6000, 16, 33, "notify", "drawn", "steady")["mismatches"] == 0
    assert _run(exe, "test", 1500, 10, 2)["mismatches"] == 0
    r = _run(exe, "test", 20000, 12, 1, "steady")               # no notifications, >= 16 384 entities: the frames whose queue stood go by the records
    assert r["mismatches"] == 0 and r["frames_by_the_records"] >= 6 and r["fast_frames"] == 0
    r = _run(exe, "test", 2000, 24, 1, "steady")                # ... a small queue is walked (one thread would lose by the records)
    assert r["mismatches"] == 0 and r["frames_by_the_records"] == 0
    assert _run(exe, "test", 1500, 10, 3, "notify")["mismatches"] == 0
    assert _run(exe, "lod", 1500, 8, 1, "notify", "drawn", "steady")["mismatches"] == 0
    assert _run(exe, "lod", 800, 8, 2)["mismatches"] == 0
    # a frame as pipeline_render renders it: shadow passes with the light's (registered) view, then the model pass
    for args in (("lod", 1500, 9, 1, "notify", "drawn", "steady", "shadow", 2), ("lod", 800, 8, 2, "shadow", 3)):
        r = _run(exe, *args)
        assert r["mismatches"] == 0 and r["shadow_passes"] > 0 and r["cull_launches_after_update"] == r["frames_the_light_moved_after_the_update"], r
    r = _run(exe, "bench", 6000, 4, 300, "notify", "drawn", "shadow", 2)
    assert r["mismatches"] == 0 and r["shadow_sets_equal"] is True and r["cull_launches_after_update"] == 0
    assert _run(exe, "edge")["mismatches"] == 0
    r = _run(exe, "bench", 6000, 4, 300, "notify", "drawn")
    assert r["mismatches"] == 0 and r["draw_reads_equal"] is True
    assert _run(exe, "recreate", 3000)["mismatches"] == 0


@pytest.mark.timeout(1500)
def test_creation_and_deletion_in_place_under_asan_ubsan():
    """Entities made and deleted while the queue is NOT walked (gpu_scene_entity_created / _deleting; the mirror's
    clapgpu_scene_entity_new_placed / _delete_placed): tombstone records, lanes and addresses reused by the next entity,
    growth tiles, the per-slot counters of the drawn policy, the draw list by slot -- the places where a freed entity3d or a
    recycled slot would show.  `comeandgo`: entities come and go in the frames that are not walked; `plain`: what the game
    makes is what the binding can place (default hook, listed behind its parent)."""
    exe = _build("asan")
    for args in (("test", 2500, 16, 1, "notify", "drawn", "comeandgo", "plain"), ("test", 2000, 40, 7, "notify", "comeandgo", "plain"),
                 ("test", 300, 80, 5, "notify", "drawn", "comeandgo", "plain"), ("test", 2500, 16, 1, "notify", "drawn", "comeandgo")):
        r = _run(exe, *args)
        assert r["mismatches"] == 0 and r["placed_in_layout"] > 0 and r["removed_in_place"] > 0, (args, r)
    assert _run(exe, "lod", 1500, 10, 3, "notify", "drawn", "comeandgo", "plain")["mismatches"] == 0
    r = _run(exe, "bench", 6000, 12, 300, "notify", "drawn", "churn", 40)
    assert r["mismatches"] == 0 and r["draw_reads_equal"] is True
    # (the first frame with an edit is walked and makes room: one of the two warm-up frames)
    assert r["fast_frames"] == 12 and r["retiles"] == 0 and r["placed_in_layout"] >= 470 and r["removed_in_place"] >= 470, r
    # the same frames through a walk and a re-tile (the switch a maintainer has): same bits
    r = _run(exe, "bench", 6000, 6, 300, "notify", "drawn", "churn", 40, env={"GPU_SCENE_INCREMENTAL": "0"})
    assert r["mismatches"] == 0 and r["fast_frames"] == 0 and r["placed_in_layout"] == 0


@pytest.mark.timeout(1500)
def test_recycled_entity_addresses_without_a_sanitizer():
    """The sanitizers' allocators never hand a freed block out again soon, malloc does at once: a deleted entity3d's address
    is the next new entity's.  The same checker WITHOUT a sanitizer: a record looked up by address must not be taken for
    the entity it knew (found here: a new entity of the same model, updated on the spot like instantiate_entity does --
    xform.updated cleared -- kept the DELETED entity's transform on the device, in a walked frame; the deletion
    notification now marks the record)."""
    exe = _build("plain")
    for args in (("test", 5000, 16, 2), ("test", 5000, 16, 2, "notify"), ("test", 2500, 16, 1, "notify", "drawn", "comeandgo", "plain"),
                 ("test", 300, 80, 5, "notify", "drawn", "comeandgo"), ("test", 20000, 10, 9, "notify", "drawn", "comeandgo", "plain")):
        assert _run(exe, *args)["mismatches"] == 0, args
    r = _run(exe, "bench", 20000, 12, 300, "notify", "drawn", "churn", 60)
    assert r["mismatches"] == 0 and r["fast_frames"] == 12 and r["draw_reads_equal"] is True
    # every worker pass from a few hundred entities on (the thresholds are environment knobs): the orderings the passes rely on
    forced = {"GPU_SCENE_THREADS": "6", "GPU_SCENE_MIRROR_PAR_MIN": "200", "GPU_SCENE_SCATTER_PAR_MIN": "100"}
    for args in (("test", 200000, 12, 11, "notify", "drawn", "comeandgo", "plain"), ("test", 17000, 8, 705, "notify", "drawn", "comeandgo"),
                 ("test", 4000, 12, 720, "notify", "steady"), ("test", 17000, 8, 731, "steady")):
        assert _run(exe, *args, env=forced)["mismatches"] == 0, args


@pytest.mark.timeout(1800)
def test_animation_particle_character_and_light_bindings_under_the_sanitizers():
    """The four bindings beside gpu-scene.c -- gpu-anim.inc.c (pools packed per model, the joints' write-back over the worker
    pool), gpu-particles.inc.c (mapped staging, the struct particle write-back on the workers), gpu-character.inc.c,
    gpu-light.inc.c -- had never run under a sanitizer: tests/c/fake_clapgpu_anim.c gives their device entry points a CPU
    body (the oracle's pose / particles / light grid), and `clap_dropin anim | particles | characters | lights` run here
    under ASan + UBSan, then under TSan with the worker paths forced on from a few dozen joints / particles
    (GPU_ANIM_PAR_MIN, GPU_PARTICLES_PAR_MIN).  The fake computes with the oracle, so the reference's bits still have to
    come out everywhere."""
    exe = _build("asan")
    for args in (("anim", 40, 24, 6, 1), ("anim", 300, 64, 8, 2, "notify"), ("anim", 30, 200, 4, 3), ("particles", 12, 200, 8, 1),
                 ("particles", 3, 100, 6, 4), ("characters", 60, 10, 1), ("characters", 400, 12, 2, "notify"), ("lights", 12, 1)):
        r = _run(exe, *args)
        assert r["mismatches"] == 0 and r.get("differing_objects", 0) == 0 and r.get("stream_draws_agree", True), (args, r)
    exe = _build("tsan")
    forced = {"GPU_SCENE_THREADS": "6", "GPU_ANIM_THREADS": "6", "GPU_ANIM_PAR_MIN": "64", "GPU_PARTICLES_PAR_MIN": "512"}
    for args in (("anim", 60, 24, 8, 3, "notify"), ("anim", 600, 32, 5, 4), ("particles", 40, 128, 8, 2), ("particles", 80, 1024, 4, 2),
                 ("characters", 300, 8, 3, "notify"), ("lights", 6, 2)):
        r = _run(exe, *args, env=forced)
        assert r["mismatches"] == 0 and r.get("differing_objects", 0) == 0 and r.get("stream_draws_agree", True), (args, r)


@pytest.mark.timeout(1800)
def test_api_orderings_fuzzed_under_asan():
    """`clap_dropin fuzz <seed> <ops>`: every public call of gpu-scene.h in generated orders between frames -- notifications
    (true and spurious), entities made / deleted / re-parented / updated on the spot, gpu_scene_keep, fetches, the
    write-back policy and the notification mode switched back and forth, LODs, camera and light planes, the light's view
    registered and taken off, another queue served for a frame, the binding object destroyed and made again -- then a frame,
    render passes (camera's view, light's, none) and both worlds compared.  2 500 seeds of 200 calls and 300 of 1 500, under
    ASan + UBSan, a few at a time.  Pinned: the three orderings the fuzzer found when it was written (round 6) --
    305: a topology report, then another queue's frame (rows GPU_SCATTER_DRAWN had left on the device were lost with the
    records); 77: drawn, back to all, a re-tile, then a child rebuilt in a frame that is not walked (parent_seq from counters
    nobody kept); 5016: a switch to GPU_SCATTER_ALL refused its fetch because a walk was pending, then one stale child was
    fetched before its stale parent."""
    from concurrent.futures import ThreadPoolExecutor
    exe = _build("asan")
    for seed, ops in ((305, 200), (77, 200), (5016, 1500), (1421, 200)):
        assert _run(exe, "fuzz", seed, ops)["mismatches"] == 0, seed

    # every fifth seed with a walked frame's steps 2 and 3 on the workers from the first entity up (GPU_SCENE_WALK_PAR_MIN=1:
    # classes by the chase up the ancestor chain, flags / transforms pushed in parallel, the rest in list order afterwards)
    forced = {"GPU_SCENE_WALK_PAR_MIN": "1", "GPU_SCENE_THREADS": "3"}

    def one(job):
        seed, ops = job
        r = _run(exe, "fuzz", seed, ops, timeout=300, env=forced if seed % 5 == 0 else None)
        return seed, r["mismatches"], r["frames"], r["render_passes"]
    jobs = [(s, 200) for s in range(1, 2501)] + [(s, 1500) for s in range(5001, 5301)]
    with ThreadPoolExecutor(6) as pool:
        res = list(pool.map(one, jobs))
    assert [s for s, bad, _f, _p in res if bad] == []
    assert sum(f for _s, _b, f, _p in res) > 50_000 and sum(p for _s, _b, _f, p in res) > 50_000
    # ... and the scripted game the same way (creations, deletions, re-parenting, hooks, characters, joint riders)
    for args in (("test", 2500, 12, 1, "notify", "drawn", "steady"), ("test", 2000, 40, 7, "notify", "drawn", "steady"), ("test", 1500, 10, 2),
                 ("test", 2500, 16, 1, "notify", "drawn", "comeandgo"), ("lod", 1500, 8, 1, "notify", "drawn", "steady"), ("edge",),
                 ("anim", 40, 64, 8, 3), ("characters", 200, 8, 3)):
        assert _run(exe, *args, env=forced)["mismatches"] == 0, args


def test_mirror_edits_in_place_under_asan_ubsan():
    """tests/c/test_scene.c -- the host mirror driven like CLAP's frame loop, every frame against the oracle -- linked
    against the CPU stand-in and run under the sanitizers: its four frames of clapgpu_scene_entity_new_placed /
    _delete_placed edit the standing layout (growth tiles included) without a re-tile.  Then the same twelve frames, tile and
    level layout, with every slot staged through copies and with every slot zero-copy: both frame entry points
    (clapgpu_scene_mq_update, clapgpu_scene_attached_update) on each of the mirror's three transports."""
    exe = os.path.join(OUT, "test_scene_fake")
    os.makedirs(OUT, exist_ok=True)
    import glob
    srcs = [os.path.join(ROOT, "tests", "c", "test_scene.c"), *sorted(glob.glob(os.path.join(ROOT, "clap_amd", "host", "clapgpu_scene*.c"))),
            os.path.join(ROOT, "clap_amd", "host", "clapgpu_snapshot.c"), os.path.join(ROOT, "tests", "c", "fake_clapgpu.c"),
            os.path.join(ROOT, "oracle", "entity.c"), os.path.join(ROOT, "oracle", "lod.c")]
    p = subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-fsanitize=address,undefined", "-w", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "oracle"), *srcs, "-o", exe, "-lm"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert p.returncode == 0 and "PASS" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
    assert "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr, p.stderr[-3000:]
    assert "0 edits fell back to a re-tile, 4 of 4 frames without one" in p.stdout and " 0 entities placed" not in p.stdout
    # the re-tile's passes over every handle / slot as ranges on a caller's pool (clapgpu_scene_set_parallel_for): here seven
    # ranges taken backwards from one element up -- the same layout, the same frames
    import re
    for mode in ([], ["wide"]):
        base = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", CLAPGPU_SCENE_TIMING="1")
        q = subprocess.run([exe, *mode], capture_output=True, text=True, timeout=600, env=base)
        p = subprocess.run([exe, *mode], capture_output=True, text=True, timeout=600,
                           env=dict(base, TEST_SCENE_PAR_FOR="1", CLAPGPU_SCENE_PAR_MIN="1", CLAPGPU_SCENE_RT_CHUNK="200"))
        assert p.returncode == 0 and "PASS" in p.stdout and "7 ranges, backwards" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
        assert "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr, p.stderr[-3000:]
        layouts = re.findall(r"layout ([0-9a-f]{16})", p.stderr)
        assert len(layouts) >= 4 and layouts == re.findall(r"layout ([0-9a-f]{16})", q.stderr), "slot for slot the serial re-tile's layout"
    # both frame entry points on the other two transports: staged copies (no slot is zero-copy) and mapped memory (every slot
    # is; `wide` is the level layout, whose frames export through a second launch)
    for mode in ([], ["wide"]):
        for slots, path in (("0", "staged path"), ("4294967295", "small-frame path")):
            p = subprocess.run([exe, *mode], capture_output=True, text=True, timeout=600,
                               env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", CLAPGPU_SCENE_ZERO_COPY_SLOTS=slots))
            assert p.returncode == 0 and "PASS" in p.stdout and p.stdout.count("frame ok") == 12, p.stdout[-2000:] + p.stderr[-3000:]
            assert path in p.stdout, (mode, slots, p.stdout[-2000:])
            assert "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr, p.stderr[-3000:]
    # a long run: lanes recycled, growth tiles, rows that fill up (the edit falls back, the frame re-tiles, then in place again)
    p = subprocess.run([exe, "tiles", "5", "80"], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert p.returncode == 0 and "PASS" in p.stdout and p.stdout.count("frame ok") == 88, p.stdout[-1500:] + p.stderr[-2000:]
    assert "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr, p.stderr[-3000:]


@pytest.mark.timeout(1500)
def test_worker_pool_passes_under_tsan():
    """Frames that touch >= 65 536 entities split the mirror pass (the address list), the pending-count pass and the
    write-back over the worker pool; scenes are destroyed and re-created in between (the pool's last reference goes and
    comes back: ADVICE r3's use-after-return trigger).  No data race, no lock-order inversion."""
    exe = _build("tsan")
    r = _run(exe, "bench", 140000, 2, 1000, "notify", "drawn", env={"GPU_SCENE_THREADS": "6"})
    assert r["mismatches"] == 0 and r["left_stale_per_frame"] > 0
    r = _run(exe, "bench", 140000, 2, 1000, "notify", env={"GPU_SCENE_THREADS": "6"})
    assert r["mismatches"] == 0
    r = _run(exe, "recreate", 70000, env={"GPU_SCENE_THREADS": "6"})
    assert r["mismatches"] == 0 and r["fast_frames"] > 0
    # no notifications: the queue check and the mirror pass over EVERY record on the workers
    r = _run(exe, "bench", 140000, 3, 1000, env={"GPU_SCENE_THREADS": "6"})
    assert r["mismatches"] == 0 and r["frames_by_the_records"] == 3
    # the scripted game (entities moved twice a frame, updated on the spot, made and deleted) with every pass FORCED onto the
    # workers from a few hundred entities on: found on the GPU box and pinned here -- a child updated on the host read its
    # parent's counters half-way through another worker's write-back; an entity that is twice on the address list was taken
    # by two workers at once
    forced = {"GPU_SCENE_THREADS": "6", "GPU_SCENE_MIRROR_PAR_MIN": "500", "GPU_SCENE_SCATTER_PAR_MIN": "300"}
    for args in (("test", 30000, 10, 11, "notify", "drawn", "comeandgo", "plain"), ("test", 20000, 12, 13, "notify", "drawn", "steady"),
                 ("test", 30000, 10, 12, "notify", "comeandgo"), ("test", 20000, 10, 14, "steady")):
        assert _run(exe, *args, env=forced)["mismatches"] == 0, args
    # ... with entities made and deleted between the frames: tombstone records and appended ones under the split passes
    r = _run(exe, "bench", 140000, 3, 1000, "notify", "drawn", "churn", 50, env={"GPU_SCENE_THREADS": "6"})
    assert r["mismatches"] == 0 and r["fast_frames"] == 3 and r["placed_in_layout"] > 100
