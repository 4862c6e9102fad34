/*
 * gpu-scene-pool.c -- the bindings' worker pool (one per process) and gpu_scene_par_for (gpu-scene.h); gs_par_run hands a
 * pass's jobs to the workers (shared declarations in gpu-scene-internal.h).
 */
#include "gpu-scene-internal.h"

int gs_par_threads(void)
{
    static int cached;
    if (!cached) {
        long n = sysconf(_SC_NPROCESSORS_ONLN);
        const char *env = getenv("GPU_SCENE_THREADS");           /* the passes are memory latency: they scale with the cores until DRAM says no */
        if (env && atoi(env) > 0) n = atoi(env);
        else if (n > 24) n = 24;                                 /* measured on a 128-core host: 8 -> 16 -> 24 threads 26 -> 15 -> 12 ms, 32: 14 */
        if (n > GS_MAX_THREADS) n = GS_MAX_THREADS;
        cached = n < 1 ? 1 : (int)n;
    }
    return cached;
}

/*
 * The workers are kept: created with the first frame that wants them, parked on a condition variable between passes,
 * joined by gpu_scene_done().  Created per pass (round 2) every frame of a million entities paid for fourteen thread
 * creations with cold stacks (1 M all moving: walk 18 -> 15 ms, write-back 23 -> 15 ms with the workers kept).  Waking a
 * parked worker still costs tens to hundreds of microseconds (the core has to leave its idle state), so the passes are
 * split only from GS_PAR_MIN entities up: at 10 000 entities a split pass measured four times SLOWER than one thread.
 * One pool per process: the passes of one frame follow each other, and every call of the binding is synchronous on the
 * engine's one thread.  Every binding object that may split a pass (a gpu_scene, gpu_anim, gpu_particles) holds a
 * reference (gpu_scene_pool_ref / _unref); the last one to go joins the workers.
 *
 * A pass is identified by its generation.  A worker serves exactly the generations that began after it was created:
 * it starts with `seen` = the generation current at its creation (threads are created under the pool's mutex, so no
 * pass can begin in between), and `pending` is set, under the same mutex, to the number of workers alive when the
 * generation is raised -- a thread created later never decrements a count it was not part of, and never sees the
 * function or the (stack-allocated) job array of a pass that has returned.
 */
static struct {
    pthread_t th[GS_MAX_THREADS - 1];
    int n;                                                       /* workers running */
    pthread_mutex_t mu;
    pthread_cond_t work;
    void *(*fn)(void *);
    struct par_job *jobs;
    int nt;                                                      /* jobs of the current pass (job 0 is the caller's) */
    unsigned gen;
    int pending;                                                 /* workers still busy with the current pass */
    int users;                                                   /* binding objects holding the pool */
    bool quit;
} g_pool = { .mu = PTHREAD_MUTEX_INITIALIZER, .work = PTHREAD_COND_INITIALIZER };

struct pool_arg { int me; unsigned seen; };

static void *pool_worker(void *arg)
{
    const struct pool_arg pa = *(struct pool_arg *)arg;           /* serves job me + 1 */
    free(arg);
    const int me = pa.me;
    unsigned seen = pa.seen;
    pthread_mutex_lock(&g_pool.mu);
    for (;;) {
        while (g_pool.gen == seen && !g_pool.quit) pthread_cond_wait(&g_pool.work, &g_pool.mu);
        if (g_pool.quit) break;
        seen = g_pool.gen;
        void *(*fn)(void *) = g_pool.fn;
        struct par_job *job = me + 1 < g_pool.nt ? &g_pool.jobs[me + 1] : NULL;
        pthread_mutex_unlock(&g_pool.mu);
        if (job) fn(job);
        __atomic_fetch_sub(&g_pool.pending, 1, __ATOMIC_RELEASE);
        pthread_mutex_lock(&g_pool.mu);
    }
    pthread_mutex_unlock(&g_pool.mu);
    return NULL;
}

/* called with the pool's mutex held */
static void pool_grow(int workers)
{
    while (g_pool.n < workers && g_pool.n < GS_MAX_THREADS - 1) {
        struct pool_arg *pa = malloc(sizeof(*pa));
        if (!pa) break;
        *pa = (struct pool_arg){ .me = g_pool.n, .seen = g_pool.gen };
        if (pthread_create(&g_pool.th[g_pool.n], NULL, pool_worker, pa)) { free(pa); break; }
        g_pool.n++;
    }
}

static void pool_stop(void)
{
    pthread_mutex_lock(&g_pool.mu);
    const int n = g_pool.n;
    g_pool.quit = true;
    pthread_cond_broadcast(&g_pool.work);
    pthread_mutex_unlock(&g_pool.mu);
    for (int t = 0; t < n; t++) pthread_join(g_pool.th[t], NULL);
    pthread_mutex_lock(&g_pool.mu);
    g_pool.n = 0;
    g_pool.quit = false;
    g_pool.fn = NULL; g_pool.jobs = NULL; g_pool.nt = 0;          /* nothing of a finished pass survives the workers */
    g_pool.pending = 0;
    pthread_mutex_unlock(&g_pool.mu);
}

void gpu_scene_pool_ref(void)
{
    pthread_mutex_lock(&g_pool.mu);
    g_pool.users++;
    pthread_mutex_unlock(&g_pool.mu);
}

void gpu_scene_pool_unref(void)
{
    pthread_mutex_lock(&g_pool.mu);
    const bool last = g_pool.users > 0 && --g_pool.users == 0;
    pthread_mutex_unlock(&g_pool.mu);
    if (last) pool_stop();                                       /* every call of the binding is on the engine's one thread: no pass is running */
}

void gs_par_run(void *(*fn)(void *), struct par_job *jobs, int nt)
{
    pthread_mutex_lock(&g_pool.mu);
    pool_grow(nt - 1);
    const int workers = g_pool.n;                                /* fewer than asked for if thread creation failed */
    if (workers > 0) {
        g_pool.fn = fn; g_pool.jobs = jobs; g_pool.nt = nt < workers + 1 ? nt : workers + 1;
        __atomic_store_n(&g_pool.pending, workers, __ATOMIC_RELAXED);     /* exactly the workers that will see this generation */
        g_pool.gen++;
        pthread_cond_broadcast(&g_pool.work);
    }
    pthread_mutex_unlock(&g_pool.mu);
    fn(&jobs[0]);
    for (int t = workers + 1; t < nt; t++) fn(&jobs[t]);        /* jobs no worker exists for */
    while (__atomic_load_n(&g_pool.pending, __ATOMIC_ACQUIRE) > 0)   /* the caller has nothing else to do: spin */
        __builtin_ia32_pause();
}

static void *par_range(void *arg)
{
    struct par_job *j = arg;
    if (!j->cursor) { j->range_fn(j->ctx, j->lo, j->hi); return NULL; }
    for (;;) {                                                   /* the next piece nobody has taken yet */
        const uint32_t k = __atomic_fetch_add(j->cursor, j->grain, __ATOMIC_RELAXED);
        if (k >= j->total) break;
        j->range_fn(j->ctx, k, j->total - k < j->grain ? j->total : k + j->grain);
    }
    return NULL;
}

/* fn(ctx, lo, hi) over a partition of [0, n) on the binding's workers and the caller.  The ranges are handed out piece by
 * piece from a shared cursor (about eight pieces a thread), not cut into one range per thread: the hosts this runs on are
 * shared, a worker that loses its core for a millisecond would otherwise hold the whole pass for it (measured: the same
 * pass 2x slower on a busy box than on a quiet one with one range a thread).  Nothing may depend on the cut: every range
 * function here writes what its indices own. */
void gpu_scene_par_for(void (*fn)(void *, uint32_t, uint32_t), void *ctx, uint32_t n, int threads)
{
    if (threads > gs_par_threads()) threads = gs_par_threads();
    if (threads < 2 || n < (uint32_t)threads) { fn(ctx, 0, n); return; }
    struct par_job jobs[GS_MAX_THREADS] = { 0 };
    uint32_t cursor = 0;
    uint32_t grain = n / ((uint32_t)threads * GS_PAR_PIECES);
    if (grain && grain < 64) grain = 64;
    for (int t = 0; t < threads; t++)
        jobs[t] = (struct par_job){ .lo = (uint32_t)((uint64_t)n * t / threads), .hi = (uint32_t)((uint64_t)n * (t + 1) / threads),
                                    .range_fn = fn, .ctx = ctx, .cursor = grain ? &cursor : NULL, .total = n, .grain = grain };
    gs_par_run(par_range, jobs, threads);
}

