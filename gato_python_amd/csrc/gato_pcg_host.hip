// PCG dispatch: co-residency gate, launch arguments, XCD calibration, gato_pcg, tune, status, recover.
#include <vector>

#include "gato_solver.h"

// ---- co-residency gate (A12: check_sms + cudaLaunchCooperativeKernel in the reference, gato_utils.cuh:829-854,
// gato_pcg.cuh:502-526).  The workgroups of a multi-workgroup persistent launch hand data to each other inside the
// launch, so all of them must be resident at once.  One launch alone always is (W <= CUs, one workgroup per CU); two
// launches on two streams of one process could each get half their workgroups and spin until the time-out.  Every
// such launch therefore records an event, and a launch that would not fit beside the launches still in flight on OTHER
// streams of the same device first makes its stream wait for them.  (Kernels of foreign processes cannot be seen here:
// that case ends in the bounded time-out and gato_solver_recover.)
namespace {
struct InFlight { hipEvent_t ev; int cus; hipStream_t st; int device; };
std::mutex g_gate_mu;
std::vector<InFlight> g_inflight;
std::vector<InFlight> g_free_events;      // recycled events, kept with the device they were created on
}  // namespace

namespace gato {
// held from the admission check over the launch to the record of its event: two host threads must not both find the chip free and
// both launch (round 5: four threads with a solver and a stream each ran into hand-off time-outs - check, then act, was not atomic)
std::mutex g_launch_mu;

int gate_before(int device, int num_cus, int need, hipStream_t st)
{
    std::lock_guard<std::mutex> lock(g_gate_mu);
    size_t w = 0;
    for (size_t i = 0; i < g_inflight.size(); ++i) {
        if (hipEventQuery(g_inflight[i].ev) == hipSuccess) g_free_events.push_back(g_inflight[i]);
        else g_inflight[w++] = g_inflight[i];
    }
    g_inflight.resize(w);
    int busy = 0;
    for (const InFlight &f : g_inflight)
        if (f.device == device && f.st != st) busy += f.cus;
    if (busy + need > num_cus) {
        for (const InFlight &f : g_inflight)
            if (f.device == device && f.st != st) GATO_HIP_CHECK(hipStreamWaitEvent(st, f.ev, 0));
    }
    return GATO_OK;
}

int gate_after(int device, int need, hipStream_t st)
{
    std::lock_guard<std::mutex> lock(g_gate_mu);
    hipEvent_t ev = nullptr;
    for (size_t i = 0; i < g_free_events.size(); ++i)
        if (g_free_events[i].device == device) {          // an event belongs to the device it was created on
            ev = g_free_events[i].ev;
            g_free_events[i] = g_free_events.back();
            g_free_events.pop_back();
            break;
        }
    if (!ev) GATO_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    GATO_HIP_CHECK(hipEventRecord(ev, st));
    g_inflight.push_back(InFlight{ev, need, st, device});
    return GATO_OK;
}
}  // namespace gato

// One-XCD launches (xcd_pack): the hand-off granules live in one place in memory and the eight XCDs are not equally far
// from it - measured 3.00 (best XCD) to 3.27 us (worst) per iteration at 14/7/512 f32, 3.10 to 3.37 at 14/7/1024, the
// order depending on where this solver's hand-off area happened to land, stable for the life of the solver
// (tools/xcd_sel_check.py).  The hosting XCD of a geometry is therefore MEASURED: two rounds of eight short trial launches
// (16 iterations each, the second round timed with HIP events; ~1 ms in all, host-blocking), the fastest XCD is kept.
// This happens in gato_solver_tune() only - called by gato_solver_create for the geometry the solver's defaults plan,
// and by the caller again after changing geometry options - on the solver's OWN buffers (work vectors as lambda, a
// scratch iters / status / eta word): the enqueue-only entries (gato_pcg, gato_linsys_device, ...) never calibrate, never
// wait on the host and never touch caller buffers for it; a geometry without a measurement runs on XCD 0.
static int calibrate_xcd(gato_solver *s, const PcgLaunch &a0, bool cg1, hipStream_t st, int *best, bool *measured)
{
    *best = 0;
    *measured = false;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); return GATO_OK; }
    if (cap != hipStreamCaptureStatusNone || a0.max_iters < 4) return GATO_OK;
    if (!s->ev_cal0) {
        GATO_HIP_CHECK(hipEventCreate(&s->ev_cal0));
        GATO_HIP_CHECK(hipEventCreate(&s->ev_cal1));
    }
    PcgLaunch t = a0;
    t.max_iters = a0.max_iters < 16 ? a0.max_iters : 16;
    t.exit_tol = 0.0;
    t.eta_hist = nullptr;
    t.dz = nullptr;
    t.lambda0 = nullptr;
    t.stamps = nullptr; t.diag = 0; t.ablate = 0;
    t.timeout_ticks = 2000000ull;                       // 20 ms: a trial never waits the solver's 2 s
    t.ev_start = s->ev_cal0; t.ev_stop = s->ev_cal1;
    const unsigned need = 2u * (unsigned)t.max_iters + 8u;
    if (s->pcg_epoch > 0xFFFFFFFFu - 17u * need - 64u) {                    // counter about to wrap: start over on zeroed granules
        GATO_HIP_CHECK(hipMemsetAsync(s->slots, 0, s->slots_bytes, st));
        s->pcg_epoch = 0;
    }
    float best_ms = 0.f;
    for (int pass = 0; pass < 2; ++pass) {
        for (int sel = 0; sel < 8; ++sel) {
            t.xcd_sel = sel;
            t.epoch0 = s->pcg_epoch;
            s->pcg_epoch += need;
            if (++s->pcg_launch_id <= 0) s->pcg_launch_id = 1;
            t.launch_id = s->pcg_launch_id;
            int rc;
            {
                std::lock_guard<std::mutex> launch_lock(g_launch_mu);
                if ((rc = gate_before(s->device, s->num_cus, s->num_cus, st))) return rc;
                rc = cg1 ? s->ops->pcg_cg1(t, st) : s->ops->pcg_resident(t, st);
                if (rc == GATO_OK) rc = gate_after(s->device, s->num_cus, st);
            }
            if (rc) return rc;
            GATO_HIP_CHECK(hipEventSynchronize(s->ev_cal1));
            float ms = 0.f;
            GATO_HIP_CHECK(hipEventElapsedTime(&ms, s->ev_cal0, s->ev_cal1));
            // a 16-iteration trial is ~50 us: one that took 10 ms sat in a hand-off (the CUs are shared with another process,
            // its spin bound is the trial time-out) - give up, the launches run on XCD 0, instead of paying 16 time-outs
            if (ms > 10.f) { *best = 0; return GATO_OK; }
            if (pass == 1 && (sel == 0 || ms < best_ms)) { best_ms = ms; *best = sel; }
        }
    }
    *measured = true;
    return GATO_OK;
}

// Asked by pcg_one, by the pre-check of the re-solve and by gato_solver_tune.
PcgDecision pcg_decide(const gato_solver &s, const PcgOpts &o, int batch, bool capturing)
{
    PcgDecision d;
    d.mode = o.mode;
    d.refusal = PCG_GO;
    const int plan_batch = batch > 1 ? batch : s.d.B;      // a launch by launch run of a batch still plans as that batch
    // pcg_variant: 1 = single-reduction recurrence (opt-in, gato_pcg_cg1.hip)
    const bool cg1 = s.pcg_variant == 1 && d.mode != GATO_PCG_STREAMING && !o.warm &&
                     plan_cg1(s, s.d.K, &d.g) && (batch == 1 || d.g.groups == 1);
    const bool fits = cg1 || plan_resident(s, o, s.d.K, plan_batch, false, &d.g);
    if (d.mode == GATO_PCG_AUTO) d.mode = fits ? GATO_PCG_RESIDENT : GATO_PCG_STREAMING;
    if (d.mode != GATO_PCG_RESIDENT) return d;
    // A launch captured into a graph is REPLAYED with the arguments of the capture.  That is fine for a one-workgroup solve
    // (nothing in it depends on the launch's number), but not for what draws fresh values per launch: the hand-off epochs of
    // the multi-workgroup launches (on replay the granules already hold them: polls would pass on stale payloads) and the
    // dz flag of the helper blocks (it would already equal the launch id: dz from an unfinished lambda).  So while the
    // stream is being captured the helper blocks do not do dz (the dz launch of its own follows), and a launch that needs
    // epochs is refused - the streaming kernels (pcg_mode = 2) replay correctly.
    if (!fits) d.refusal = PCG_NO_FIT;
    else if (capturing && (d.g.groups > 1 || s.cl.on)) d.refusal = PCG_NO_CAPTURE;
    return d;
}

// calibration key of a one-XCD geometry
static long long xcd_key(const gato_solver *s, const PcgGeometry &g)
{
    return ((long long)g.groups << 32) | ((long long)g.threads << 8) | (g.cg1 ? 2 : 0) | (s->esz == 8 ? 1 : 0) | 4 | (g.dpp ? 8 : 0);
}

// The launch of a resident decision: arguments, a fresh range of hand-off epochs, the launch id, whether dz rides along.
static int pcg_build(gato_solver *s, const PcgOpts &o, const PcgGeometry &geo, const void *d_S, const void *d_Pinv, const void *d_gamma,
                     void *d_lambda, double exit_tol, int max_iters, int *d_iters, int batch, int rhs, bool capturing,
                     hipStream_t st, PcgLaunch *out)
{
    const int groups = geo.groups, threads = geo.threads;
    const bool cg1 = geo.cg1;
    PcgLaunch &a = *out;
    memset(&a, 0, sizeof(a));
    a.S_bd = d_S; a.P_bd = d_Pinv; a.gamma = d_gamma; a.lambda = d_lambda;
    a.lambda0 = o.warm ? d_lambda : nullptr;      // in place: every lane reads its lambda0 first
    a.K = s->d.K; a.max_iters = max_iters; a.exit_tol = exit_tol;
    a.batch = batch;
    a.rhs = rhs;
    a.pair = geo.pair;
    // (the single-reduction kernel and the LDS-DMA ring keep the plain launch: option coop_launch serves the resident / semi-resident launches)
    a.coop = s->coop_launch && groups > 1 && batch == 1 && !cg1 && geo.semi != 3;
    // (every lane of the launch loads rows 2 tid, 2 tid + 1 resp. its own row: all of them must lie inside a column of the image)
    if (s->img_fresh && !s->no_image && batch == 1 && d_S == s->Sbd && d_Pinv == s->Pbd &&
        ((geo.pair == 1 && 2 * threads <= s->img_ld) || (geo.pair == 2 && s->plan.mixed_rows <= s->img_ld))) {
        a.imgS = s->imgS; a.imgP = s->imgP; a.img_ld = s->img_ld;
    }
    a.semi = geo.semi;
    a.dpp_rows = geo.dpp;
    // option xcd_pack: -1 = auto (default): up to 32 workgroups are placed on ONE XCD (measured 15-20 % faster hand-offs:
    // 14/7/512 f32 3.96 -> 3.11 us/iteration); spreading over 2..7 XCDs measured no better than the plain grid, so
    // auto leaves larger launches alone.  0 = off, 1..7 = force that many XCDs (tools/xcd_pack_check.py).
    a.xcd_pack = 0;
    if (s->xcd_pack != 0 && batch == 1 && groups > 1) {
        const int need = (groups + 31) / 32;
        if (s->xcd_pack < 0) a.xcd_pack = need == 1 ? 1 : 0;
        else a.xcd_pack = (s->xcd_pack >= need && s->xcd_pack < 8) ? s->xcd_pack : 0;
    }
    if (a.semi) a.xcd_pack = 0;
    a.xcd_sel = s->xcd_sel;
    a.wave_pub = s->wave_pub;
    if (a.xcd_pack > 0 && groups > s->num_cus / 8) a.xcd_pack = 0;     // an XCD with fewer CUs than workgroups (CU mask): plain grid
    a.knots_per_wg = geo.kpw; a.groups = groups; a.threads = threads;
    a.slots = s->slots; a.iters = d_iters ? d_iters : s->iters; a.status = s->status;
    // hand-off epochs: each launch gets a fresh range (two reductions per iteration plus the initial one)
    const unsigned need = max_iters > 0x3FFFFFF0 ? 0x80000000u : 2u * (unsigned)max_iters + 8u;
    if (s->pcg_epoch > 0xFFFFFFFFu - need - 8u) {            // counter about to wrap: start over on zeroed granules
        GATO_HIP_CHECK(hipMemsetAsync(s->slots, 0, s->slots_bytes, st));
        s->pcg_epoch = 0;
    }
    a.epoch0 = s->pcg_epoch;
    s->pcg_epoch += need;
    if (++s->pcg_launch_id <= 0) s->pcg_launch_id = 1;
    a.launch_id = s->pcg_launch_id;
    a.final_eta = s->final_eta;
    a.eta_hist = (s->record_eta && max_iters <= GATO_ETA_HIST_MAX) ? s->eta_hist : nullptr;
    a.timeout_ticks = (unsigned long long)s->timeout_ms * 100000ull;   // s_memrealtime runs at 100 MHz
    // one workgroup (per system) holds every lambda_k: the dz back-substitution rides in the same launch
    // (batches only: every system's workgroup does its own dz and a launch of 25 600 one-wave workgroups goes away; for
    //  ONE system the single workgroup is as latency bound as that launch was - measured 11 us in the epilogue against
    //  5.3 us + a launch gap - unless asked for with no_fuse_dz = -1)
    // (fp32 two-rows-per-lane kernel: its epilogue exists for batches)
    if (s->fz.dz && (s->no_fuse_dz < 0 || (!s->no_fuse_dz && batch > 1)) && groups == 1 && !cg1 &&
        (geo.pair != 1 || batch > 1) && !a.semi && !o.stamp) {
        a.dz_Ginv = s->fz.Ginv; a.dz_Cd = s->fz.Cd; a.dz_g = s->fz.g; a.dz = s->fz.dz; a.C = s->d.C;
    }
    // ONE system through a two-rows-per-lane one-workgroup kernel (pcg_single_f64m_kernel = BASELINE configs[1]; pcg_single_f32x2_kernel): its helper blocks - there
    // to warm the L2 - stay and do dz as soon as lambda is published: the dz launch and the gap in front of it (6.5 us of a
    // 215 us step) become ~1 us at the end of the PCG launch.  no_fuse_dz = 1 keeps the launch of its own.
    else if (s->fz.dz && !s->no_fuse_dz && batch == 1 && groups == 1 && !cg1 && (geo.pair == 2 || geo.pair == 1) && !o.stamp && !capturing) {
        a.dz_Ginv = s->fz.Ginv; a.dz_Cd = s->fz.Cd; a.dz_g = s->fz.g; a.dz = s->fz.dz; a.C = s->d.C;
        a.dz_helpers = 1; a.dz_flag = s->dz_flag;
    }
    a.ablate = s->ablate;
    a.stamps = o.stamp == 1 ? (unsigned long long *)s->sw.scalars + 8 : nullptr;
    a.diag = o.stamp;
    a.ev_start = s->time_pcg ? s->ev_pcg0 : nullptr;
    a.ev_stop = s->time_pcg ? s->ev_pcg1 : nullptr;
    return GATO_OK;
}

// Launches what pcg_build made and records it as the latest launch (options last_*).
static int pcg_launch(gato_solver *s, const PcgGeometry &geo, PcgLaunch &a, bool capturing, hipStream_t st)
{
    const int groups = geo.groups, threads = geo.threads, batch = a.batch;
    const bool cg1 = geo.cg1;
    s->last_image = a.imgS != nullptr;
    s->dz_fused = a.dz ? (a.dz_helpers ? 2 : 1) : 0;
    s->last_groups = groups; s->last_threads = threads; s->last_mode = GATO_PCG_RESIDENT;
    s->last_variant = cg1 ? 1 : 0;
    s->last_semi = a.semi; s->last_pair = geo.pair; s->last_dpp = geo.dpp;
    s->last_stream = st;
    // co-residency: a multi-workgroup launch waits for launches on other streams it would not fit beside
    // (a one-XCD launch counts as the whole chip: two of them may be dealt to the same XCD)
    const bool gated = batch == 1 && groups > 1;
    const int need_cus = a.xcd_pack > 0 ? s->num_cus : groups;
    int rc;
    // one-XCD launches: which of the eight XCDs hosts them (option xcd_sel: -1 = measured once per geometry, 0..7 fixed)
    s->last_xcd_sel = -1;
    if (a.xcd_pack > 0) {
        if (s->xcd_sel >= 0) a.xcd_sel = s->xcd_sel;
        else a.xcd_sel = s->xcd_cal_key == xcd_key(s, geo) ? s->xcd_cal_best : 0;       // not measured for this geometry: XCD 0
        s->last_xcd_sel = a.xcd_sel;
    }
    const bool gate = gated && !capturing;      // (a captured multi-workgroup launch was refused above; the gate records events)
    std::unique_lock<std::mutex> launch_lock(g_launch_mu, std::defer_lock);
    if (gate) launch_lock.lock();
    if (gate && (rc = gate_before(s->device, s->num_cus, need_cus, st))) return rc;
    rc = cg1 ? s->ops->pcg_cg1(a, st) : a.semi == 3 ? s->ops->pcg_dma(a, st) : s->ops->pcg_resident(a, st);
    if (rc == GATO_OK && gate) rc = gate_after(s->device, need_cus, st);
    return rc;
}

// The error of a refused decision (GATO_OK: it may run).
static int pcg_refused(const gato_solver *s, const PcgDecision &d)
{
    if (d.refusal == PCG_NO_FIT)
        set_error("pcg: K=%d does not fit the resident kernel on %d CUs (threads=%d groups=%d)", s->d.K,
                  s->num_cus, s->pcg_threads, s->pcg_groups);
    if (d.refusal == PCG_NO_CAPTURE)
        set_error("pcg: a persistent launch of %d workgroups cannot be captured into a graph (its hand-off epochs are launch "
                  "arguments: a replay would read stale granules); capture the streaming kernels (option pcg_mode = 2) "
                  "or a system that fits one workgroup", d.g.groups);
    return d.refusal == PCG_GO ? GATO_OK : GATO_EINVAL;
}

int pcg_one(gato_solver *s, const PcgOpts &o, const void *d_S, const void *d_Pinv, const void *d_gamma, void *d_lambda,
            double exit_tol, int max_iters, int *d_iters, int batch, hipStream_t st, int rhs)
{
    const bool capturing = o.mode != GATO_PCG_STREAMING && stream_is_capturing(st);
    const PcgDecision d = pcg_decide(*s, o, batch, capturing);
    if (pcg_refused(s, d)) return GATO_EINVAL;
    if (d.mode == GATO_PCG_RESIDENT) {
        PcgLaunch a;
        const int rc = pcg_build(s, o, d.g, d_S, d_Pinv, d_gamma, d_lambda, exit_tol, max_iters, d_iters, batch, rhs, capturing, st, &a);
        return rc ? rc : pcg_launch(s, d.g, a, capturing, st);
    }
    s->last_stream = st;
    s->last_mode = GATO_PCG_STREAMING; s->last_groups = 0; s->last_threads = 0; s->last_semi = 0; s->last_pair = 0; s->last_dpp = 0;
    s->dz_fused = 0;
    s->sw.warm_start = o.warm;
    s->sw.eta_hist = (s->record_eta && max_iters <= GATO_ETA_HIST_MAX) ? s->eta_hist : nullptr;
    if (s->time_pcg) GATO_HIP_CHECK(hipEventRecord(s->ev_pcg0, st));
    int rc = s->ops->pcg_streaming(s->d, d_S, d_Pinv, d_gamma, d_lambda, exit_tol, max_iters,
                                   d_iters ? d_iters : s->iters, s->sw, st);
    if (s->time_pcg) GATO_HIP_CHECK(hipEventRecord(s->ev_pcg1, st));
    return rc;
}

// The PCGs of the solver's B systems: one workgroup per system in a single launch when a system fits one CU; otherwise system by system
int pcg_systems(gato_solver *s, const PcgOpts &o, const void *d_S, const void *d_Pinv, const void *d_gamma, void *d_lambda,
                double exit_tol, int max_iters, int *d_iters, hipStream_t st)
{
    const int B = s->d.B;
    int *its = d_iters ? d_iters : s->iters;
    if (B == 1 || plan_one_wg_each(*s, o, B)) return pcg_one(s, o, d_S, d_Pinv, d_gamma, d_lambda, exit_tol, max_iters, its, B, st);
    const size_t e = s->esz;
    s->fz.dz = nullptr;                      // system by system: dz stays a launch of its own
    for (int b = 0; b < B; ++b) {
        int rc = pcg_one(s, o, (const char *)d_S + b * s->d.bd() * e, (const char *)d_Pinv + b * s->d.bd() * e,
                         (const char *)d_gamma + b * s->d.sk() * e, (char *)d_lambda + b * s->d.sk() * e, exit_tol,
                         max_iters, its + b, 1, st);
        if (rc) return rc;
    }
    return GATO_OK;
}

extern "C" int gato_pcg(gato_solver *s, const void *d_S, const void *d_Pinv, const void *d_gamma, void *d_lambda,
                        double exit_tol, int max_iters, int *d_iters, void *stream)
{
    return pcg_systems(s, pcg_opts(*s), d_S, d_Pinv, d_gamma, d_lambda, exit_tol, max_iters, d_iters, (hipStream_t)stream);
}

// Measures, for the geometry the solver's CURRENT options plan, which XCD should host a one-XCD launch (see above
// calibrate_xcd).  Blocking (~1 ms: 16 short launches, each waited for); runs on `stream`, reads the solver's own S / Pinv /
// gamma work buffers (whatever they hold: the launches run a fixed iteration count and their results are discarded) and
// writes only solver-owned scratch.  A no-op for batches, cluster ranks and geometries that are not one-XCD launches.
// gato_solver_create calls it once; call it again after changing pcg_threads / pcg_groups / pcg_variant / max_workgroups
// / xcd_pack if those launches should keep the measured placement (unmeasured geometries run on XCD 0: a placement
// hint only, results never depend on it).
extern "C" int gato_solver_tune(gato_solver *s, void *stream)
{
    if (!s) { set_error("solver_tune: null solver"); return GATO_EINVAL; }
    if (s->d.B != 1 || s->cl.on || s->xcd_sel >= 0 || s->pcg_mode == GATO_PCG_STREAMING) return GATO_OK;
    GATO_HIP_CHECK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    const PcgOpts o{s->pcg_mode, 0, 0};                    // cold start, no stamps
    const PcgDecision d = pcg_decide(*s, o, 1, false);     // (calibrate_xcd looks at a capture itself)
    if (pcg_refused(s, d)) return GATO_EINVAL;
    PcgLaunch a;
    int rc = GATO_OK;
    if (d.mode == GATO_PCG_RESIDENT && !(rc = pcg_build(s, o, d.g, s->Sbd, s->Pbd, s->gamma, s->sw.vecs, 0.0, 16, s->tune_iters, 1, 1, false, st, &a))) {
        s->last_xcd_sel = -1;
        if (a.xcd_pack > 0) {
            // the trial launches (scratch outputs, own events); no launch of the caller's follows
            bool measured = false;
            a.iters = s->tune_iters; a.status = s->tune_status; a.final_eta = s->tune_eta;
            rc = calibrate_xcd(s, a, d.g.cg1, st, &s->xcd_cal_best, &measured);
            s->xcd_cal_key = measured ? xcd_key(s, d.g) : 0;
            s->last_xcd_sel = measured ? s->xcd_cal_best : -1;
        }
    }
    if (rc) return rc;
    GATO_HIP_CHECK(hipStreamSynchronize(st));
    return GATO_OK;
}

// Reports a hand-off time-out of ANY PCG launch since the previous call (the status word keeps the id of the most
// recent launch that timed out; no kernel ever clears it), after synchronising the stream of the latest launch.
// The same condition is visible in-band: the launch wrote iters = -1.
extern "C" int gato_pcg_status(gato_solver *s, int *status)
{
    int v = 0;
    GATO_HIP_CHECK(hipSetDevice(s->device));
    GATO_HIP_CHECK(hipStreamSynchronize(s->last_stream));
    GATO_HIP_CHECK(hipMemcpy(&v, s->status, sizeof(int), hipMemcpyDeviceToHost));
    const bool timed_out = v != s->status_ack;
    s->status_ack = v;
    if (status) *status = timed_out ? 1 : 0;
    if (timed_out) { set_error("pcg: in-kernel hand-off timed out (launch %d)", v); return GATO_ETIMEOUT; }
    return GATO_OK;
}

// A12 fallback: if a persistent launch of the most recent whole solve (gato_linsys_device / _blocks) gave up on a
// hand-off - its workgroups were not co-resident, e.g. another process held the CUs - the PCG is re-run through the
// streaming kernels (no inter-workgroup hand-off inside a launch, any residency) and dz is recomputed: a slower
// correct answer instead of an error.  Synchronises `stream`.  *recovered = 1 when that happened.
extern "C" int gato_solver_recover(gato_solver *s, int *recovered, void *stream)
{
    if (recovered) *recovered = 0;
    s->last_fallback = 0;
    int st_ = 0;
    const int rc = gato_pcg_status(s, &st_);
    if (rc == GATO_OK) return GATO_OK;
    if (rc != GATO_ETIMEOUT || !s->lc.valid) return rc;
    PcgOpts o = pcg_opts(*s);
    o.mode = GATO_PCG_STREAMING;
    s->d.k_lo = s->d.k_hi = 0;
    int rc2 = s->lc.rhs > 0 ? pcg_rhs(s, o, s->lc.rhs, s->lc.gamma, s->lc.lam, s->lc.exit_tol, s->lc.max_iters, s->lc.its, (hipStream_t)stream)
                            : pcg_systems(s, o, s->lc.S, s->lc.P, s->lc.gamma, s->lc.lam, s->lc.exit_tol, s->lc.max_iters, s->iters, (hipStream_t)stream);
    if (rc2) return rc2;
    if (s->lc.rhs > 0) rc2 = dz_rhs(s, s->lc.rhs, s->lc.g, s->lc.lam, s->lc.dz, (hipStream_t)stream);
    else if (s->lc.dz) rc2 = gato_compute_dz(s, s->Ginv, s->lc.Cd, s->lc.g, s->lc.lam, s->lc.dz, stream);
    if (rc2) return rc2;
    GATO_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    s->last_fallback = 1;
    if (recovered) *recovered = 1;
    return GATO_OK;
}

