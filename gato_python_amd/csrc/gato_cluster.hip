// Knot-sharded PCG protocol (gato_shard_pcg_*) and the multi-GPU cluster (gato_cluster_*).
#include <cstdlib>
#include <vector>

#include "gato_solver.h"

extern "C" int gato_shard_pcg_done(gato_solver *s, int *done, void *stream)
{
    GATO_HIP_CHECK(hipMemcpyAsync(done, s->sw.done, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    GATO_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return GATO_OK;
}

// ---- knot-sharded PCG (multi-GPU) ------------------------------------------------------------------
static char *ghost_ptr(gato_solver *s, int vec /*0 r, 1 p*/, int pp, int side)
{
    return s->ghosts + ((size_t)((vec * 2 + pp) * 2 + side) * s->d.S) * s->esz;
}

static void shard_vectors(gato_solver *s, char *r[2], char *p[2], char **ups, char **rt)
{
    const size_t sk = s->d.sk() * s->esz;
    char *v = (char *)s->sw.vecs;
    r[0] = v; r[1] = v + sk; p[0] = v + 2 * sk; p[1] = v + 3 * sk; *ups = v + 4 * sk; *rt = v + 5 * sk;
}

static void shard_common(gato_solver *s, StreamStep &a)
{
    memset(&a, 0, sizeof(a));
    a.K = s->sh.k1 - s->sh.k0;
    a.max_iters = s->sh.max_iters; a.exit_tol = s->sh.exit_tol; a.done = s->sw.done; a.iters = s->iters;
    a.first_global = s->sh.k0 == 0; a.last_global = s->sh.k1 == s->d.K;
}

extern "C" int gato_shard_pcg_init(gato_solver *s, int rank, int nranks, int k0, int k1, const void *d_S,
                                   const void *d_Pinv, const void *d_gamma, double exit_tol, int max_iters,
                                   void *d_send, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const int S = s->d.S;
    const size_t e = s->esz;
    if (rank < 0 || rank >= nranks || k0 < 0 || k1 <= k0 || k1 > s->d.K || (rank == 0) != (k0 == 0) ||
        (rank == nranks - 1) != (k1 == s->d.K)) {
        set_error("shard_pcg_init: bad shard rank=%d/%d knots [%d,%d) of %d", rank, nranks, k0, k1, s->d.K);
        return GATO_EINVAL;
    }
    s->sh.rank = rank; s->sh.nranks = nranks; s->sh.k0 = k0; s->sh.k1 = k1; s->sh.max_iters = max_iters;
    s->sh.exit_tol = exit_tol;
    s->sh.S_full = (const char *)d_S; s->sh.P_full = (const char *)d_Pinv; s->sh.gamma_full = (const char *)d_gamma;
    s->sh.grid = s->ops->stream_grid(k1 - k0, s->sw.max_groups);
    GATO_HIP_CHECK(hipMemsetAsync(s->lambda, 0, s->d.sk() * e, st));
    char *r[2], *p[2], *ups, *rt;
    shard_vectors(s, r, p, &ups, &rt);
    StreamStep a;
    shard_common(s, a);
    a.M = s->sh.P_full + (size_t)k0 * 3 * S * S * e;
    a.a_old = s->sh.gamma_full + (size_t)k0 * S * e;
    a.gh_a_left = s->sh.gamma_full + (size_t)(k0 > 0 ? k0 - 1 : 0) * S * e;
    a.gh_a_right = s->sh.gamma_full + (size_t)(k1 < s->d.K ? k1 : 0) * S * e;
    a.gh_new_left = ghost_ptr(s, 0, 0, 0); a.gh_new_right = ghost_ptr(s, 0, 0, 1);
    a.a_new = r[0]; a.y = rt; a.lam = (char *)s->lambda + (size_t)k0 * S * e;
    a.part_out = s->sw.partials; a.it = 0;
    int rc;
    if ((rc = s->ops->stream_step(0, a, s->sh.grid, st))) return rc;
    return s->ops->stream_pack(s->sw.partials, s->sh.grid, rt, k1 - k0, d_send, st);
}

extern "C" int gato_shard_pcg_phase_a(gato_solver *s, int it, const void *d_recvB_cur, const void *d_recvB_prev,
                                      void *d_send, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const int S = s->d.S, REC = 2 * S + 1, rank = s->sh.rank;
    const size_t e = s->esz;
    char *r[2], *p[2], *ups, *rt;
    shard_vectors(s, r, p, &ups, &rt);
    const int pi = it & 1;
    StreamStep a;
    shard_common(s, a);
    a.M = s->sh.S_full + (size_t)s->sh.k0 * 3 * S * S * e;
    a.a_old = p[pi ^ 1]; a.b = rt; a.a_new = p[pi]; a.y = ups; a.it = it;
    a.part_num = d_recvB_cur; a.num_n = s->sh.nranks; a.num_stride = REC;
    a.part_den = d_recvB_prev; a.den_n = s->sh.nranks; a.den_stride = REC;
    const char *rb = (const char *)d_recvB_cur;                 // r~ blocks of the neighbours
    a.gh_b_left = rb + ((size_t)(rank > 0 ? rank - 1 : 0) * REC + 1 + S) * e;
    a.gh_b_right = rb + ((size_t)(rank + 1 < s->sh.nranks ? rank + 1 : 0) * REC + 1) * e;
    a.gh_a_left = ghost_ptr(s, 1, pi ^ 1, 0); a.gh_a_right = ghost_ptr(s, 1, pi ^ 1, 1);
    a.gh_new_left = ghost_ptr(s, 1, pi, 0); a.gh_new_right = ghost_ptr(s, 1, pi, 1);
    char *PA = (char *)s->sw.partials + (size_t)3 * s->sw.max_groups * e;
    a.part_out = PA;
    int rc;
    if ((rc = s->ops->stream_step(1, a, s->sh.grid, st))) return rc;
    return s->ops->stream_pack(PA, s->sh.grid, ups, s->sh.k1 - s->sh.k0, d_send, st);
}

extern "C" int gato_shard_pcg_phase_b(gato_solver *s, int it, const void *d_recvB_cur, const void *d_recvA,
                                      void *d_send, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const int S = s->d.S, REC = 2 * S + 1, rank = s->sh.rank;
    const size_t e = s->esz;
    char *r[2], *p[2], *ups, *rt;
    shard_vectors(s, r, p, &ups, &rt);
    const int ri = it & 1, pi = it & 1;
    StreamStep a;
    shard_common(s, a);
    a.M = s->sh.P_full + (size_t)s->sh.k0 * 3 * S * S * e;
    a.a_old = r[ri]; a.b = ups; a.a_new = r[ri ^ 1]; a.y = rt; a.it = it;
    a.lam = (char *)s->lambda + (size_t)s->sh.k0 * S * e; a.p_cur = p[pi];
    a.part_num = d_recvB_cur; a.num_n = s->sh.nranks; a.num_stride = REC;   // eta(it)
    a.part_den = d_recvA; a.den_n = s->sh.nranks; a.den_stride = REC;       // v(it)
    const char *ra = (const char *)d_recvA;                     // upsilon blocks of the neighbours
    a.gh_b_left = ra + ((size_t)(rank > 0 ? rank - 1 : 0) * REC + 1 + S) * e;
    a.gh_b_right = ra + ((size_t)(rank + 1 < s->sh.nranks ? rank + 1 : 0) * REC + 1) * e;
    a.gh_a_left = ghost_ptr(s, 0, ri, 0); a.gh_a_right = ghost_ptr(s, 0, ri, 1);
    a.gh_new_left = ghost_ptr(s, 0, ri ^ 1, 0); a.gh_new_right = ghost_ptr(s, 0, ri ^ 1, 1);
    a.part_out = s->sw.partials;
    int rc;
    if ((rc = s->ops->stream_step(2, a, s->sh.grid, st))) return rc;
    return s->ops->stream_pack(s->sw.partials, s->sh.grid, rt, s->sh.k1 - s->sh.k0, d_send, st);
}

extern "C" int gato_shard_pcg_finish(gato_solver *s, const void *d_recvB_last, void *d_lambda_full_out, int *d_iters,
                                     void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    int rc = s->ops->stream_finish(d_recvB_last, s->sh.nranks, 2 * s->d.S + 1, s->sh.exit_tol, s->sh.max_iters - 1,
                                   s->sw.done, s->iters, s->final_eta, nullptr, st);
    if (rc) return rc;
    if (d_lambda_full_out && d_lambda_full_out != s->lambda)
        GATO_HIP_CHECK(hipMemcpyAsync(d_lambda_full_out, s->lambda, s->d.sk() * s->esz, hipMemcpyDeviceToDevice, st));
    if (d_iters && d_iters != s->iters)
        GATO_HIP_CHECK(hipMemcpyAsync(d_iters, s->iters, sizeof(int), hipMemcpyDeviceToDevice, st));
    return GATO_OK;
}

// ---- multi-GPU cluster: the persistent PCG launch with a device-initiated cross-GPU hand-off level --------------------
// NEW work: the reference is single-device (gato_utils.cuh:831) and has no communication layer.
// One process per GPU.  Every rank owns a MIRROR - a few KB of fine-grained device memory, IPC-shared - into which the
// peers store {epoch, payload} granules with system-scope stores over xGMI; a rank only ever polls its own mirror.  See
// pcg_resident_kernel<..., MR = true> for the protocol.  RCCL (gato_shard_pcg_*) stays as the portable fallback.
// Mirrors are RECYCLED inside the process, never handed back to the allocator while it lives: pages that were mapped uncached
// and come back as ordinary (cached) device memory after hipFree can read stale - round 5, tools/cluster_fuzz.py: a solver arena
// allocated over a freed uncached mirror read whole 128-B lines of zeros where the mirror's polled lines had been (P / gamma rows
// of a later solve; only with the uncached kind, not with fine-grained or plain mirrors).  A few hundred KB per mirror.
namespace {
struct MirrorBuf { void *p; size_t bytes; int device, kind; };
std::mutex g_mirror_mu;
std::vector<MirrorBuf> g_mirror_pool;

void *mirror_take(int device, int kind, size_t bytes, size_t *got)
{
    std::lock_guard<std::mutex> lock(g_mirror_mu);
    for (size_t i = 0; i < g_mirror_pool.size(); ++i) {
        const MirrorBuf b = g_mirror_pool[i];
        if (b.device == device && b.kind == kind && b.bytes >= bytes && b.bytes <= 4 * bytes) {
            g_mirror_pool[i] = g_mirror_pool.back();
            g_mirror_pool.pop_back();
            *got = b.bytes;
            return b.p;
        }
    }
    return nullptr;
}

void mirror_give(void *p, int device, int kind, size_t bytes)
{
    std::lock_guard<std::mutex> lock(g_mirror_mu);
    g_mirror_pool.push_back(MirrorBuf{p, bytes, device, kind});
}
}  // namespace

static int cluster_alloc(gato_solver *s)
{
    const char *env = getenv("GATO_XMEM");           // uncached | finegrained | plain (default: first that works)
    const int first = env ? (!strcmp(env, "plain") ? 2 : !strcmp(env, "finegrained") ? 1 : 0) : 0;
    void *p = nullptr;
    s->cl.alloc_bytes = s->cl.bytes;
    for (int kind = first; kind < 3; ++kind) {
        if ((p = mirror_take(s->device, kind, s->cl.bytes, &s->cl.alloc_bytes))) { s->cl.mem_kind = kind; break; }
        hipError_t e = kind == 0 ? hipExtMallocWithFlags(&p, s->cl.bytes, hipDeviceMallocUncached)
                     : kind == 1 ? hipExtMallocWithFlags(&p, s->cl.bytes, hipDeviceMallocFinegrained)
                                 : hipMalloc(&p, s->cl.bytes);
        if (e == hipSuccess && p) { s->cl.mem_kind = kind; break; }
        (void)hipGetLastError();
        p = nullptr;
    }
    if (!p) { set_error("cluster: cannot allocate the %zu-byte mirror", s->cl.bytes); return GATO_EHIP; }
    s->cl.local = (unsigned long long *)p;
    GATO_HIP_CHECK(hipMemset(p, 0, s->cl.bytes));
    GATO_HIP_CHECK(hipDeviceSynchronize());
    return GATO_OK;
}

extern "C" int gato_cluster_knot_range(int K, int rank, int nranks, int *k0, int *k1)
{
    if (nranks < 1 || rank < 0 || rank >= nranks || K < nranks) {
        set_error("cluster: cannot shard %d knots over %d ranks (rank %d)", K, nranks, rank);
        return GATO_EINVAL;
    }
    const int base = K / nranks, extra = K % nranks;           // balanced contiguous ranges, as dist.knot_ranges
    *k0 = rank * base + (rank < extra ? rank : extra);
    *k1 = *k0 + base + (rank < extra ? 1 : 0);
    return GATO_OK;
}

extern "C" int gato_cluster_create(gato_solver *s, int rank, int nranks, void *ipc_handle_out)
{
    if (s->d.B != 1 || nranks > GATO_MAX_RANKS) {
        set_error("cluster: one system per solver, at most %d ranks", GATO_MAX_RANKS);
        return GATO_EINVAL;
    }
    int k0, k1, rc;
    if ((rc = gato_cluster_knot_range(s->d.K, rank, nranks, &k0, &k1))) return rc;
    GATO_HIP_CHECK(hipSetDevice(s->device));
    gato_cluster_destroy(s);
    memset(&s->cl, 0, sizeof(s->cl));
    s->as.valid = 0;                  // the cluster entries assemble shards into the same workspace
    s->cl.rank = rank; s->cl.nranks = nranks; s->cl.k0 = k0; s->cl.k1 = k1;
    // two-level area (2 parities), then the flat area: a slot for each of up to 256 workgroups of the whole cluster
    s->cl.flat_off = align_up((size_t)2 * pcg_xslot_granules(s->d.S, (int)s->esz), 16);
    // ... then the lambda ghost block a rank receives from its right neighbour at the end of a launch (cluster_lambda_ghost)
    s->cl.lam_off = s->cl.flat_off + (size_t)2 * 256 * pcg_flat_slot_granules(s->d.S, (int)s->esz);
    const size_t need = (s->cl.lam_off + (size_t)pcg_lamghost_granules(s->d.S, (int)s->esz)) * 8;
    s->cl.bytes = need < 65536 ? 65536 : align_up(need, 65536);
    if ((rc = cluster_alloc(s))) return rc;
    s->cl.peer[rank] = s->cl.local;
    if (ipc_handle_out) {
        hipIpcMemHandle_t h;
        GATO_HIP_CHECK(hipIpcGetMemHandle(&h, s->cl.local));
        static_assert(sizeof(h) == 64, "ipc handle size");
        memcpy(ipc_handle_out, &h, sizeof(h));
    }
    return GATO_OK;
}

extern "C" void *gato_cluster_local_mirror(gato_solver *s) { return s->cl.local; }

// handles: nranks x 64 bytes in rank order (other processes' mirrors are opened through them), and / or ptrs: mirrors
// that are plain device pointers in THIS process (ranks living in one process).  After this call and BEFORE the first
// gato_cluster_pcg every rank must pass a host-level barrier (torch.distributed.barrier): the mirrors are zeroed here.
extern "C" int gato_cluster_connect(gato_solver *s, const void *ipc_handles, void *const *ptrs)
{
    if (!s->cl.local) { set_error("cluster_connect: gato_cluster_create first"); return GATO_EINVAL; }
    GATO_HIP_CHECK(hipSetDevice(s->device));
    for (int r = 0; r < s->cl.nranks; ++r) {
        if (r == s->cl.rank) continue;
        if (ptrs && ptrs[r]) { s->cl.peer[r] = (unsigned long long *)ptrs[r]; continue; }
        if (!ipc_handles) { set_error("cluster_connect: no mirror given for rank %d", r); return GATO_EINVAL; }
        hipIpcMemHandle_t h;
        memcpy(&h, (const char *)ipc_handles + (size_t)r * sizeof(h), sizeof(h));
        void *p = nullptr;
        GATO_HIP_CHECK(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
        s->cl.peer[r] = (unsigned long long *)p;
        s->cl.opened[r] = true;
    }
    GATO_HIP_CHECK(hipMemcpy(s->cl_tab, s->cl.peer, sizeof(void *) * GATO_MAX_RANKS, hipMemcpyHostToDevice));
    s->cl.on = 1;
    return gato_cluster_rewind(s);                 // fresh epoch spaces on both levels (every rank does the same, then the caller's barrier)
}

// The hand-off epochs of a cluster only grow (32 bits; a launch takes 2 max_iters + 8 of them on every rank alike), and a mirror
// cannot be re-zeroed in stream order as the one-GPU slots are: a peer that is already in its next launch may have stored into it.
// So the epoch space is renewed by the CALLER, on every rank at the same solve: when gato_cluster_launches_left says that the next
// launch does not fit (the counters run in lock-step, every rank sees it at the same call), each rank waits for its own
// launches, all ranks pass a host barrier (nobody stores into a mirror any more), each rank calls gato_cluster_rewind (zeroes its
// mirror and its level-1 slots, counters back to 0), all pass a second barrier, and the solves go on.  dist.ClusterPCG does this.
extern "C" int gato_cluster_launches_left(gato_solver *s, int max_iters, long long *left)
{
    if (!s->cl.on || !left) { set_error("cluster_launches_left: gato_cluster_connect first"); return GATO_EINVAL; }
    if (max_iters < 0) { set_error("cluster_launches_left: max_iters must be >= 0 (got %d)", max_iters); return GATO_EINVAL; }
    const unsigned long long need = max_iters > 0x3FFFFFF0 ? 0x80000000ull : 2ull * (unsigned)max_iters + 8ull;
    const unsigned long long top = 0xFFFFFFFFull - need - 8ull;
    const unsigned long long used = s->cl.xepoch;          // (the level-1 counter of a rank renews itself in stream order: gato_cluster_pcg)
    *left = used > top ? 0 : (long long)((top - used) / need) + 1;
    return GATO_OK;
}

extern "C" int gato_cluster_rewind(gato_solver *s)
{
    if (!s->cl.local) { set_error("cluster_rewind: gato_cluster_create first"); return GATO_EINVAL; }
    GATO_HIP_CHECK(hipSetDevice(s->device));
    GATO_HIP_CHECK(hipDeviceSynchronize());
    GATO_HIP_CHECK(hipMemset(s->cl.local, 0, s->cl.bytes));
    GATO_HIP_CHECK(hipMemset(s->slots, 0, s->slots_bytes));
    GATO_HIP_CHECK(hipDeviceSynchronize());
    s->pcg_epoch = 0;
    s->cl.xepoch = 0;
    return GATO_OK;
}

extern "C" int gato_cluster_destroy(gato_solver *s)
{
    if (!s) return GATO_OK;
    for (int r = 0; r < GATO_MAX_RANKS; ++r)
        if (s->cl.opened[r] && s->cl.peer[r]) (void)hipIpcCloseMemHandle(s->cl.peer[r]);
    if (s->cl.local) mirror_give(s->cl.local, s->device, s->cl.mem_kind, s->cl.alloc_bytes);      // kept for the next cluster
    memset(&s->cl, 0, sizeof(s->cl));
    return GATO_OK;
}

extern "C" int gato_cluster_fits(gato_solver *s, int *groups, int *threads)
{
    if (!s->cl.local) { set_error("cluster_fits: gato_cluster_create first"); return GATO_EINVAL; }
    PcgGeometry g;                                  // (all zero where the rank's knots do not fit)
    cluster_plan(*s, pcg_opts(*s), s->cl.rank, &g);
    if (groups) *groups = g.groups;
    if (threads) *threads = g.threads;
    return GATO_OK;
}

// One rank's part of a PCG solve sharded over the cluster: d_S / d_Pinv / d_gamma / d_lambda are FULL-system arrays
// (block row 0 first) of which this rank reads / writes the rows of its range only (variant 1: Pinv and gamma also on the
// neighbouring knots, see cluster_plan_cg1 / gato_cluster_linsys).  Every rank must call it with the same exit_tol and
// max_iters; the launches synchronise with each other on the device (bounded spins), never on the host.  d_iters: as gato_pcg
// (-1 = a hand-off timed out).  d_lambda holds this rank's slice on return - and, on every rank but the last, the right
// neighbour's first block at row k_end (cluster_lambda_ghost: what the dz of this rank's last knot needs).
extern "C" int gato_cluster_pcg(gato_solver *s, const void *d_S, const void *d_Pinv, const void *d_gamma, void *d_lambda,
                                double exit_tol, int max_iters, int *d_iters, void *stream)
{
    if (!s->cl.on) { set_error("cluster_pcg: gato_cluster_connect first"); return GATO_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    // a captured launch would be REPLAYED with the epochs of the capture: stale granules would pass the polls (see pcg_decide)
    if (stream_is_capturing(st)) {
        set_error("cluster_pcg: a cluster launch cannot be captured into a graph (its hand-off epochs are launch arguments)");
        return GATO_EINVAL;
    }
    if (max_iters < 0) { set_error("cluster_pcg: max_iters must be >= 0 (got %d)", max_iters); return GATO_EINVAL; }
    const PcgOpts o = pcg_opts(*s);
    PcgGeometry geo;
    int flat_total = 0, flat_base = 0;
    const bool cg1 = cluster_plan_cg1(*s, o, &geo, &flat_total, &flat_base);
    if (!cg1 && !cluster_plan(*s, o, s->cl.rank, &geo)) {
        set_error("cluster_pcg: %d knots per rank do not fit a persistent launch on %d CUs", s->cl.k1 - s->cl.k0, s->num_cus);
        return GATO_EINVAL;
    }
    const unsigned need = max_iters > 0x3FFFFFF0 ? 0x80000000u : 2u * (unsigned)max_iters + 8u;
    if (s->cl.xepoch > 0xFFFFFFFFu - need - 8u) {
        set_error("cluster_pcg: epoch space used up - renew it on every rank (gato_cluster_launches_left / gato_cluster_rewind between two barriers)");
        return GATO_EINVAL;
    }
    if (s->pcg_epoch > 0xFFFFFFFFu - need - 8u) {
        GATO_HIP_CHECK(hipMemsetAsync(s->slots, 0, s->slots_bytes, st));
        s->pcg_epoch = 0;
    }
    PcgLaunch a;
    memset(&a, 0, sizeof(a));
    a.S_bd = d_S; a.P_bd = d_Pinv; a.gamma = d_gamma; a.lambda = d_lambda;
    a.lambda0 = o.warm ? d_lambda : nullptr;
    a.K = s->d.K; a.max_iters = max_iters; a.exit_tol = exit_tol;
    a.batch = 1; a.semi = geo.semi; a.dpp_rows = geo.dpp;
    a.wave_pub = s->wave_pub;
    a.knots_per_wg = geo.kpw; a.groups = geo.groups; a.threads = geo.threads;
    a.slots = s->slots; a.iters = d_iters ? d_iters : s->iters; a.status = s->status;
    a.epoch0 = s->pcg_epoch; s->pcg_epoch += need;
    a.xepoch0 = s->cl.xepoch; s->cl.xepoch += need;
    a.lam_off = s->cl.lam_off;
    a.lam_tag = a.xepoch0 + need;                   // > every epoch of this launch, < every epoch of the next: unique, never 0
    if (++s->pcg_launch_id <= 0) s->pcg_launch_id = 1;
    a.launch_id = s->pcg_launch_id;
    a.final_eta = s->final_eta;
    a.eta_hist = (s->record_eta && max_iters <= GATO_ETA_HIST_MAX) ? s->eta_hist : nullptr;
    a.timeout_ticks = (unsigned long long)s->timeout_ms * 100000ull;
    a.k_begin = s->cl.k0; a.k_end = s->cl.k1; a.rank = s->cl.rank; a.nranks = s->cl.nranks;
    a.xslots = s->cl.local;
    a.xpeer = s->cl_tab;
    // flat exchange when the whole cluster has at most 256 workgroups and every rank runs the plain resident variant
    // (cluster_plan_flat) or every rank the single-reduction one (cluster_plan_cg1 has counted them)
    a.flat = 0;
    if (s->cluster_flat != 0 && s->cl.nranks > 1 && (cg1 ? flat_total <= 256 : !a.semi && cluster_plan_flat(*s, o, &flat_total, &flat_base))) {
        a.flat = 1; a.flat_groups = flat_total; a.flat_base = flat_base; a.flat_off = s->cl.flat_off;
    }
    s->cl.last_flat = a.flat;
    // (One-XCD placement of a rank's <= 32 workgroups, as one-GPU launches get, was measured for cluster launches in round 5 and
    //  not kept: a cluster of one rank at 14/7/512 f32 3.47 -> 3.35 us per iteration, fp64 5.2 -> 5.8; with 8 / 4 ranks sharing a chip
    //  the flat exchange (5.74 / 4.88) beats two levels with packed level 1 (6.67 / 5.43).  What separates these launches from the
    //  2.2 us of the plain launch at the same knot count is the lean hand-off with workgroup-scope stores, which the MR kernels'
    //  level 1 does not have - DESIGN_LOG.md R5.7.)
    a.ev_start = s->time_pcg ? s->ev_pcg0 : nullptr;
    a.ev_stop = s->time_pcg ? s->ev_pcg1 : nullptr;
    s->last_groups = geo.groups; s->last_threads = geo.threads; s->last_mode = GATO_PCG_RESIDENT; s->last_variant = cg1 ? 1 : 0;
    s->last_semi = geo.semi; s->last_pair = geo.pair; s->last_dpp = geo.dpp; s->last_stream = st;
    // the launches of a cluster wait for EACH OTHER: they are never queued behind one another (ranks sharing a device
    // exist in tests only), but they count for the other launches of this process
    int rc;
    std::lock_guard<std::mutex> launch_lock(g_launch_mu);
    if ((rc = cg1 ? s->ops->pcg_cg1(a, st) : a.semi == 3 ? s->ops->pcg_dma(a, st) : s->ops->pcg_resident(a, st))) return rc;
    return gate_after(s->device, geo.groups, st);
}

// One rank's part of a WHOLE solve sharded over the cluster (gato_linsys, gpu_library.cu:25-83, on this rank's knot range): the
// stage kernels on the knots its PCG shard reads (S / Pinv rows k0..k1-1 complete: S[k].right comes from the Schur step of knot
// k+1 and the stair blocks need theta^-1 of both neighbours, gamma on k0-1..k1 - hence CSR scatter + inversions on [k0-2-h, k1+1+h),
// Schur steps on [k0-1-h, k1+1+h), stair on [k0-h, k1+h); h = 1 for the single-reduction recurrence, whose edge workgroups also
// multiply with the neighbouring knots' Pinv rows), the rank's cluster launch, and dz on [k0, k1) - lambda_{k1} arrives inside
// the launch (cluster_lambda_ghost), so NOTHING crosses the host or a collective between assembly, PCG and dz: one call, a handful
// of enqueues.  CSR inputs, d_g, d_c: the full system (replicated); d_lambda / d_dz: full-length arrays of which the rank writes
// its rows (lambda: + row k1).  Work buffers: the solver's own.
extern "C" int gato_cluster_linsys(gato_solver *s, const int *d_G_row, const int *d_G_col, const void *d_G_val, const int *d_C_row,
                                   const int *d_C_col, const void *d_C_val, const void *d_g, const void *d_c, double exit_tol,
                                   int max_iters, double rho, void *d_lambda, void *d_dz, int *d_iters, void *stream)
{
    if (!s->cl.on) { set_error("cluster_linsys: gato_cluster_connect first"); return GATO_EINVAL; }
    if (s->precon_mode != GATO_PRECON_STAIR) { set_error("cluster_linsys: the stair preconditioner only"); return GATO_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    const int K = s->d.K, k0 = s->cl.k0, k1 = s->cl.k1;
    const int h = (s->pcg_variant == 1 && !s->true_warm_start) ? 1 : 0;           // wide enough for either recurrence the launch may take
    auto clip = [&](int k) { return k < 0 ? 0 : (k > K ? K : k); };
    auto range = [&](int lo, int hi) { s->d.k_lo = clip(lo); s->d.k_hi = clip(hi); if (s->d.k_hi == 0) s->d.k_lo = 0; };
    int rc;
    const bool ts = s->time_stages != 0;
    if (ts) GATO_HIP_CHECK(hipEventRecord(s->ev_stage[0], st));
    // (the fused one-launch assembly of small one-GPU solves was tried here for small shards - 512 knots, what K = 4096 over 8 GPUs
    //  gives - and measured no better: 31 against 28 us outside the loop, tools/cluster_step_time.py; the stage kernels stay)
    range(k0 - 2 - h, k1 + 1 + h);
    rc = s->ops->convert(s->d, d_G_row, d_G_col, d_G_val, d_C_row, d_C_col, d_C_val, rho, s->G_dense, s->C_dense, nullptr, st);
    // (form_schur inverts the Q_k, R_k of its knot range first and then runs the Schur steps on the same range: the step of the
    //  range's first knot reads an inverse outside the range and only writes rows k0-2-h of S / Pinv, which nobody reads)
    if (!rc) rc = s->ops->form_schur(s->d, s->G_dense, s->C_dense, d_g, d_c, s->Sbd, s->Pbd, s->gamma, s->Ginv, false, st);
    if (!rc) { range(k0 - h, k1 + h); rc = s->ops->form_ss(s->d, s->Sbd, s->Pbd, st); }
    s->d.k_lo = s->d.k_hi = 0;
    if (rc) return rc;
    if (ts) GATO_HIP_CHECK(hipEventRecord(s->ev_stage[1], st));
    if ((rc = gato_cluster_pcg(s, s->Sbd, s->Pbd, s->gamma, d_lambda, exit_tol, max_iters, d_iters, stream))) return rc;
    if (ts) GATO_HIP_CHECK(hipEventRecord(s->ev_stage[2], st));
    s->d.k_lo = k0; s->d.k_hi = k1;
    rc = s->ops->compute_dz(s->d, s->Ginv, s->C_dense, d_g, d_lambda, d_dz, st);
    s->d.k_lo = s->d.k_hi = 0;
    if (ts && !rc) GATO_HIP_CHECK(hipEventRecord(s->ev_stage[3], st));
    return rc;
}
