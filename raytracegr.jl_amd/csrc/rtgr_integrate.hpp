// rtgr_integrate.hpp — the integrate kernel of the production trace pipeline:
//     prepare (camera ray, queue key, u̇(y0), initial dt) -> [order scan/scatter] -> integrate<FAR> -> integrate<NEAR>
//     -> resolve                                                              (rtgr_pipeline.hpp: launch_trace)
//
// Why a pipeline instead of one loop per ray (the simple tile kernel, trace_kernel in rtgr_tile.hpp, keeps that shape):
//   * rays need 27…991 Tsit5 step attempts inside one image; a wave that owns 64 fixed rays idles until
//     its longest ray ends, and each ray's end-of-life episode (bracketed root-find on the dense output, colouring,
//     next ray's camera set-up) would run with one lane active;
//   * so the integrate kernel treats a wave as a pool of 64 ray slots: a lane whose ray has ended writes a small
//     EVENT RECORD (the position polynomial of its last step) to HBM, and is re-filled from a global ray queue on the
//     next iteration — a wavefront ballot finds the free lanes, which take ids from the wave's slice of the queue;
//   * everything that happens once per ray and diverges — root-finding, the colouring rule with its acos/atan2 —
//     runs afterwards in the resolve kernel with every lane busy; the camera (make_canvas) runs before, likewise;
//   * the ContinuousCallback scan (8 interior samples per accepted step) is replaced, while a ray is out of reach of
//     every object, by a rigorous bound (FAR pass); rays within reach are handed to the NEAR pass (full scan);
//   * the queue is ordered longest-expected-first so that few rays per lane still balance (order_* kernels).
//   HBM traffic of the hand-offs: ≈ 1 kB per ray, against ≈ 0.23 Mflop of integration per ray.
//
// Step body (per lane, registers only):
//   * Nyström form: since ẋ = u (src/RayTraceGR.jl:360) stage positions are x + h c_s u + h² Σ A2[s][l] k_l — only the
//     seven acceleration 4-vectors k_l are stored (28 scalars), not the 7 x 8 stage derivatives;
//   * a fresh ray's u̇(y0) and Hairer initial dt (2 RHS evaluations) are computed by prepare_kernel, one thread per
//     ray, into the same 16-scalar record the FAR pass uses to hand a ray over — the integrate loop has ONE way to
//     start a ray and no per-ray set-up code of its own (an in-loop "init pseudo-step" ran its ~200 extra
//     instructions for the whole wave in the ~26 % of iterations in which some lane had just been refilled);
//   * error norm, PI controller and initial-dt formula run in f32 on the (otherwise idle) f32 VALU/transcendental
//     path; they only steer the step size — the state arithmetic is all R (f64);
//   * ContinuousCallback (NEAR / FULL): the position interpolant is put in polynomial form once per accepted step and
//     evaluated at the 8 interior sample points θ = j/9; distances are evaluated object-major so
//     each object's parameters are fetched once per block of sample points.
#pragma once
#include "rtgr_objects.hpp"
#include "rtgr_tsit5_tables.hpp"

#ifndef RTGR_GHOST_LANES
#define RTGR_GHOST_LANES 1  // lanes without a ray run the step's control block too (few-lane VALU instructions are 2.4 x dearer)
#endif
#ifndef RTGR_WAVES_PER_SIMD_GENERIC
#define RTGR_WAVES_PER_SIMD_GENERIC 2  // generic dual-number RHS: ~270 registers wanted; 2 waves with a small spill beat 1 wave (measured 6.72 vs 6.22 Gstep/s)
#endif
#ifndef RTGR_LDSK_GENERIC
#define RTGR_LDSK_GENERIC 0   // generic RHS kernels keep k[1..5] in LDS (experiment: see DESIGN §4.2 "LDS stage storage")
#endif
#ifndef RTGR_LDSK_GRID4
#define RTGR_LDSK_GRID4 1     // the time-dependent grid's Float64 kernels keep k[1..5] in LDS: beside the 4-D interpolant they spill otherwise (§4.11)
#endif
#ifndef RTGR_LDSK_SPIN_FAR
#define RTGR_LDSK_SPIN_FAR 0  // the a != 0 FAR pass keeps k[1..5] in LDS (experiment, with RTGR_WAVES_PER_SIMD_SPIN_FAR=4)
#endif
#ifndef RTGR_WAVES_PER_SIMD_SPIN_FAR
#define RTGR_WAVES_PER_SIMD_SPIN_FAR RTGR_WAVES_PER_SIMD_FAR
#endif
#ifndef RTGR_WAVES_PER_SIMD_GENERIC_F32
#define RTGR_WAVES_PER_SIMD_GENERIC_F32 3  // generic dual-number RHS in Float32: half the register bytes of the f64 kernel
#endif
// metric sampled on a grid (RTGR_GRID): the interpolant's 40 accumulators + a row of 40 samples beside the integrator's
// state want ~400 registers; at the generic kernels' 2 (Float64) / 3 (Float32) waves per SIMD the passes spilled 600-850 / 420-550 bytes
// per lane to scratch (tests/test_build_checks.py allows 64), at ONE wave they keep everything in VGPRs + AGPRs with no scratch
#ifndef RTGR_WAVES_PER_SIMD_GRID
#define RTGR_WAVES_PER_SIMD_GRID 1
#endif
#ifndef RTGR_WAVES_PER_SIMD_GRID_F32
#define RTGR_WAVES_PER_SIMD_GRID_F32 1
#endif
// time-dependent grid (RTGR_GRID4): four slices of a row in flight and 50 accumulators — one wave per SIMD as well
#ifndef RTGR_WAVES_PER_SIMD_GRID4
#define RTGR_WAVES_PER_SIMD_GRID4 1
#endif
#ifndef RTGR_WAVES_PER_SIMD_GRID4_F32
#define RTGR_WAVES_PER_SIMD_GRID4_F32 1
#endif
#ifndef RTGR_WAVES_PER_SIMD_FAR
#define RTGR_WAVES_PER_SIMD_FAR 3  // the FAR pass has no sample-point arrays: <=168 registers, three waves per SIMD
#endif
#ifndef RTGR_WAVES_PER_SIMD_F32
#define RTGR_WAVES_PER_SIMD_F32 3  // Float32 NEAR / FULL passes: 146-158 registers, three waves fit (2048²: 4.02 -> 3.50 ms; four: 3.82)
#endif
#ifndef RTGR_WAVES_PER_SIMD
#define RTGR_WAVES_PER_SIMD 2  // 2 -> <=256 VGPR+AGPR per lane; 1 -> the whole 512-entry file
#endif

namespace rtgr {

// What integrate_kernel<…> is BUILT for (its __launch_bounds__) and what the host sizes its launches by (rtgr_pipeline.hpp), in one place
template <class R, int METRIC, bool SPIN = false> constexpr int waves_per_simd_of(int mode) {
    if (Sampled<R, METRIC>::time_dependent) return sizeof(R) == 8 ? RTGR_WAVES_PER_SIMD_GRID4 : RTGR_WAVES_PER_SIMD_GRID4_F32;
    if (Sampled<R, METRIC>::is) return sizeof(R) == 8 ? RTGR_WAVES_PER_SIMD_GRID : RTGR_WAVES_PER_SIMD_GRID_F32;
    if (METRIC >= RTGR_GENERIC_BASE) return sizeof(R) == 8 ? RTGR_WAVES_PER_SIMD_GENERIC : RTGR_WAVES_PER_SIMD_GENERIC_F32;
    if (mode == MODE_FAR) return sizeof(R) == 8 ? (SPIN ? RTGR_WAVES_PER_SIMD_SPIN_FAR : RTGR_WAVES_PER_SIMD_FAR) : 4;
    return sizeof(R) == 8 ? RTGR_WAVES_PER_SIMD : RTGR_WAVES_PER_SIMD_F32;
}
// … and whether it keeps the stage accelerations k[1..5] in LDS (integrate_body's LDSK)
template <class R, int METRIC, bool SPIN> constexpr bool ldsk_of(int mode) {
    if (Sampled<R, METRIC>::time_dependent) return sizeof(R) == 8 && RTGR_LDSK_GRID4 != 0;
    if (METRIC >= RTGR_GENERIC_BASE) return RTGR_LDSK_GENERIC != 0;
    return SPIN && mode == MODE_FAR && RTGR_LDSK_SPIN_FAR != 0;
}

// FAR pass: append the wave's collected early-list entries (LDS) to the global list; ONE atomic for all of them
constexpr uint32_t RTGR_EARLY_BUF = 128;
template <class R>
RTGR_DEV void flush_early(const IntegrateArgs<R>& A, const uint32_t* buf, uint32_t cnt, uint32_t lane) {
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(A.ctrl + 6, (unsigned long long)cnt);
    base = uniform64(base);
    for (uint32_t i = lane; i < cnt; i += 64) A.early[base + i] = buf[i];
}

// The kernel body is a device function so that run-time generated units (user metrics, rtgr_user_unit.hip.in) can
// wrap it in extern "C" kernels of their own.
template <class R, int METRIC, bool SPIN, bool NPTS10, int MODE, bool LDSK = false>
RTGR_DEV void integrate_body(const IntegrateArgs<R>& A) {
    using N = Tsit5N<R>;
    const uint32_t lane = threadIdx.x & 63;
    // NEAR visits the early list first (ids [0, n_early) of its queue), then every ray id, picking up the rays flagged
    // for it that are not on the list.  The early rays then run packed together from the start of the pass — all far from
    // every object most of the time, so their waves skip the scan — instead of sitting one or two to a wave of
    // short-lived rays and keeping it alive when the queue is empty (measured before: the median wave ended at 2.2 ms,
    // the pass at 3.3 ms).
    uint64_t n_early = 0;
    if (MODE == MODE_NEAR && A.early) {  // (wave-uniform for the compiler too: it sets the loop's exit)
        const unsigned long long c = A.ctrl[6];
        n_early = uniform64(c);
    }
    const uint64_t total = A.n + n_early;
    unsigned long long* const queue = (MODE == MODE_NEAR) ? A.ctrl + 1 : A.ctrl;
    const MetricK<R> MK = scene_consts<R, METRIC>(A.sc);
    const R reltol = A.opt.reltol, abstol = A.opt.abstol;
    const R t0 = A.opt.lambda0, t1 = A.opt.lambda1, dtmax = uniform_(A.opt.lambda1 - A.opt.lambda0);
    const float igamma = 1.0f / 0.9f, qmin_inv = 5.0f, qmax_inv = 0.1f;
    const float lq_init = -13.287712379549449f;  // log2(qoldinit = 1e-4)
    const float beta1 = 0.14f, beta2 = 0.08f;
    const int npts = (int)A.opt.interp_points;
    const R eps = sizeof(R) == 8 ? R(2.220446049250313e-16) : R(1.1920929e-7);
    const R t1_snap = uniform_(t1 - R(16) * eps * rmaxabs<R>(t0, t1));   // below this λ the snap-to-λ1 test cannot hold
    // (the NEAR pass's scan mask, below: one bit per 2^mask_shift neighbours of the device list — one per object up to 64 objects)
    const uint32_t mask_shift = A.sc.nobj > 64u ? 32u - (uint32_t)__builtin_clz((A.sc.nobj - 1u) >> 6) : 0u;

    int state = L_FREE;
    bool exhausted = false;
    R x[4], u[4], k0[4];  // loop-carried ray state: position, velocity, FSAL acceleration u̇(x, u)
    R t = t0, dt = R(0), ps = R(0);
    float lq = lq_init;
    uint64_t idx = 0;
    uint32_t nacc = 0, nrej = 0, nacc0 = 0, c_maxnear = 0, safe_streak = 0;
    uint32_t c_rays = 0, c_acc = 0, c_rej = 0, c_ev = 0, c_int = 0, c_nf = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) { x[q] = R(1); u[q] = R(0); k0[q] = R(0); }

    // wave-local slice of the global ray queue: ids [q_next, q_end) were popped with ONE atomic and are dealt to lanes as
    // they free up.  (One device-scope atomic per ray on a single word saturates at ~90 M/s chip-wide — measured: it
    // stalled the FAR pass 5x — so waves pop up to RTGR_QUEUE_CHUNK ids at a time; fewer when the whole job is only a few
    // hundred rays per wave, or the last chunks would unbalance the waves.)
    uint64_t q_next = 0, q_end = 0;
    bool first_pop = true;
    bool first_early = true, early_done = false;  // NEAR: the early list's own cursor (ctrl[7])
    __shared__ uint32_t early_buf[RTGR_EARLY_BUF];  // one wave per workgroup: private to the wave (used by the FAR pass)
    __shared__ R ldsk_mem[LDSK ? 20 * 64 : 1];
    // (volatile: re-read at each use instead of being kept live in registers; address space 3: ds_read / ds_write — a generic pointer
    // would make them flat accesses, which wait on vmcnt behind every outstanding global load)
    volatile __attribute__((address_space(3))) R* const ldsk = (__attribute__((address_space(3))) R*)(ldsk_mem + lane);
    uint32_t e_cnt = 0;                             // entries in early_buf (wave-uniform)
#ifdef RTGR_ROOT_STATS
    const unsigned long long dbg_t0 = wall_clock64();
    unsigned long long dbg_iters = 0, dbg_rays = 0;
#endif
    const unsigned long long qchunk = A.queue_chunk;
    // Wave ages.  A SIMD's arbiter issues from its OLDEST ready wave first, and a persistent grid never renews its
    // waves: measured (round 1; its successor is tools/wave_timeline.py on a -DRTGR_ROOT_STATS build) 2.9 us per iteration for the first-launched
    // third of the FAR pass's workgroups, 5-7 us for the second, 14 us for the youngest (40 us on the 4-wave grid).
    // Throughput does not care, the tail of a small launch does: a young wave that holds rays of 950 steps needs
    // the whole pass for them.  So (a) the head of the longest-first queue goes to the low workgroup indices (first
    // pop by index), and (b) in small launches (fair_shift != 0) the waves of a SIMD take turns at the top priority
    // (s_setprio, time slices of 2^fair_shift clocks): per-iteration times 4.1-7.3 us instead of 2.9-14.5, FAR pass
    // 7.08 -> 6.31 ms at 1 M rays; no effect at 2-4 M rays, 1 % SLOWER at 16.8 M (where there is no tail to win and the
    // rotation only disturbs the arbiter) and 15 % slower at <= 0.5 M (one or two rays per lane: the old waves should
    // race through the longest ones), hence by launch size.  Serving the queue from both ends — old
    // waves from the head, young ones from the tail — was worse at every size: the tail-servers then run
    // shortest-first, the worst order inside a wave.
    const uint32_t n_simd = A.n_simd ? A.n_simd : 1024u;              // SIMDs of the device (MI355X: 256 CUs x 4)
    const uint32_t n_cls = (gridDim.x + n_simd - 1u) / n_simd;        // waves per SIMD of this launch
    const uint32_t my_cls = blockIdx.x / n_simd;
    const bool fair = A.fair_shift != 0u && n_cls > 1u;
    for (;;) {
        if (fair) {
            const uint32_t turn = (my_cls + (uint32_t)(__builtin_readcyclecounter() >> A.fair_shift)) % n_cls;
            switch (turn) {  // s_setprio takes an immediate
                case 0: __builtin_amdgcn_s_setprio(3); break;
                case 1: __builtin_amdgcn_s_setprio(2); break;
                case 2: __builtin_amdgcn_s_setprio(1); break;
                default: __builtin_amdgcn_s_setprio(0); break;
            }
        }
        // [budget: refill]
        // ================= refill: free lanes take ray ids from the wave's slice of the queue ====================
        const bool resume = (MODE == MODE_NEAR || A.pick_flag != 0u);
        unsigned long long m_need = __ballot(state == L_FREE);
        while (m_need != 0ull) {
            if (q_next == q_end) {
                if (exhausted) break;
                // The FIRST pop takes exactly the ids the wave can start right away: in longest-first order the head of
                // the queue holds the long rays, and ids parked in a wave's slice would only start when one of its
                // (equally long) first rays ends — simulated makespan 1978 vs 1213 steps at 5 rays per lane.
                // ... and it takes them by WAVE INDEX, not by atomic order: queue positions [64 b, 64 b + 64) go to
                // workgroup b, the atomic head serves positions from 64 * gridDim.x on (see the note on wave ages above).
                const unsigned long long first_span = 64ull * gridDim.x;
                if (MODE == MODE_NEAR && !early_done) {
                    // the early list has a head of its own and goes out 64 entries at a time: they are long-stayers, and
                    // a 256-entry chunk would be four rounds of them one after the other in the same wave (measured:
                    // the late waves of the pass were the ones that had popped such a chunk)
                    // (… unless the list is most of the job — a distant camera, every ray shorter than near_early steps:
                    //  then it is not a list of exceptions any more and goes out in full queue chunks, or its 64-id pops
                    //  are 260 k atomics at 4096², 3 ms: tools/scheduler_check.py, camera far20)
                    const unsigned long long echunk = (n_early * 8ull > A.n) ? qchunk : 64ull;
                    unsigned long long eb = 0;
                    if (first_early) eb = echunk * blockIdx.x;
                    else if (lane == 0) eb = atomicAdd(A.ctrl + 7, echunk) + echunk * gridDim.x;
                    first_early = false;
                    eb = uniform64(eb);
                    if (eb >= n_early) { early_done = true; continue; }
                    q_next = eb;
                    q_end = (eb + echunk) < n_early ? (eb + echunk) : n_early;
                    continue;
                }
                const unsigned long long amount = first_pop ? 64ull : qchunk;
                unsigned long long base = 0;
                if (first_pop) base = 64ull * blockIdx.x;
                else if (lane == 0) base = atomicAdd(queue, amount) + first_span;
                first_pop = false;
                // wave-uniform BY CONSTRUCTION and, through readfirstlane, also for the compiler: q_next / q_end /
                // exhausted then live in SGPRs and the loop's exits are scalar branches.  (With a __shfl the compiler
                // had to treat the loop exit as divergent and copied all 12 loop-carried f64 state registers to
                // shadow registers and back at the latch: 41 v_mov per iteration, 4.7 % of the kernel's instructions.)
                base = uniform64(base);
                base += n_early;  // positions [0, n_early) are the early list's
                q_next = base < total ? base : total;
                q_end = (base + amount) < total ? (base + amount) : total;
                if (base + amount >= total) exhausted = true;
                if (q_next == q_end) break;
            }
            const uint64_t avail = q_end - q_next;
            const uint32_t rank = mask_rank(m_need, lane);
            if (state == L_FREE && rank < avail) {
                const uint64_t w = q_next + rank;
                // A resuming pass (NEAR, hand-back rounds) visits every ray id and picks up the rays flagged for it.
                uint64_t id = resume ? w : (A.order ? (uint64_t)A.order[w] : w);
                bool take = true;
                if (resume) {
                    const bool listed = MODE == MODE_NEAR && w < n_early;
                    if (MODE == MODE_NEAR) id = listed ? (uint64_t)A.early[w] : w - n_early;
                    // ONE word decides: which sweep a ray belongs to is part of its flag.  (Deciding it from the step count
                    // in meta[0] raced with the wave that finishes the ray and overwrites meta[0..2] word by word: 3 rays in
                    // 4 M were traced twice — found by tools/stress_determinism.py.)
                    take = A.meta[id * 3 + 2] == (listed ? META_HANDED_EARLY : A.pick_flag);
                }
                if (take) {
                    idx = id;
                    state = L_TAKEN;
                }
            }
            const uint32_t cnt = (uint32_t)__builtin_popcountll(m_need);
            q_next += (cnt < avail) ? cnt : avail;
            m_need = __ballot(state == L_FREE);
        }
        // Every ray starts from a 16-scalar record {x, u, u̇, t, dt, sign(min_distance), log2 q_old}: written by
        // prepare_kernel for a fresh ray (u̇(y0) and the Hairer initial dt), by the FAR pass for a ray it hands over.
        // (The loads, like the commit at the end of the step, are a plain conditional assignment at the top level of the
        // loop body: assigned inside nested divergent regions, the 12 f64 state registers were shadow-copied at every
        // region entry, at the loop latch and at the loop header — 85 v_mov per iteration.)
#ifdef RTGR_ROOT_STATS
        dbg_iters++;
        dbg_rays += __builtin_popcountll(__ballot(state == L_TAKEN));
#endif
        if (state == L_TAKEN) {
            const R* hd = A.hand + idx * HAND_W;
#pragma unroll
            for (int q = 0; q < 4; q++) { x[q] = hd[q]; u[q] = hd[4 + q]; k0[q] = hd[8 + q]; }
            t = hd[12]; dt = hd[13]; ps = hd[14]; lq = (float)hd[15];
            nacc = resume ? A.meta[idx * 3] : 0u;
            nrej = resume ? A.meta[idx * 3 + 1] : 0u;
            nacc0 = nacc;
            safe_streak = 0;
            state = L_RUN;
        }
        if (exhausted && q_next == q_end && state == L_FREE) state = L_EXIT;
        // The refill loop above only gives up when the queue is exhausted, so a wave without a running lane is done.
        // (One exit and one back-edge: a `continue` here was a second latch path and cost a round trip of phi copies.)
        if (__ballot(state == L_RUN) == 0ull) break;

        // [budget: stage sums]
        // ================= one Tsit5 attempt per runnable lane ====================================================
        // The seven stages run in UNIFORM control flow: a lane without a ray computes along with h = 0 on whatever
        // state it holds (a VALU instruction costs the same with 1 or 64 lanes active) and nothing it computes is
        // used.  Only the decisions and side effects below are per-lane.
        const bool run = (state == L_RUN);
        bool commit = false;
        bool list_it = false;  // FAR: this lane's ray goes on the early list (set at hand-over)
        R xn[4], un[4], k[7][4];  // k[l] = acceleration at stage l+1 (k[0] is the FSAL slot, k[6] the next one)
        // LDSK (SURVEY §7.4 "k-stage storage in LDS if VGPR > 256"; BASELINE config 4's "LDS-tiled variant"): the stage
        // accelerations k[1..5] — 20 scalars, 40 VGPRs in f64 — live in LDS between the stage that produces them and the
        // stage sums / error estimate / reach bound that read them; slot (l, q) of lane i is word ((l−1)·4 + q)·64 + i, so
        // every access of a wave is 64 consecutive scalars (conflict-free ds_read/write_b64)
#define KL(l, q) ((LDSK && (l) >= 1 && (l) <= 5) ? (R)ldsk[(((l) - 1) * 4 + (q)) * 64] : k[l][q])
#define KSTORE(l)                                                                   \
        if constexpr (LDSK) {                                                       \
            _Pragma("unroll") for (int q_ = 0; q_ < 4; q_++) ldsk[(((l) - 1) * 4 + q_) * 64] = k[l][q_]; \
        }
#pragma unroll
        for (int q = 0; q < 4; q++) k[0][q] = k0[q];
        {
            if (run) dt = rmin(dt, t1 - t);
            const R h = run ? dt : R(0);
            const R h2 = h * h;
            R X[3], U[4];
            // x^t at the stage: formed only for a user metric that was not declared stationary (such a metric was
            // traced frozen at t = 0 — the reference evaluates christoffel(metric, x) at the full 4-position, :358-363)
            constexpr bool TDEP = needs_stage_time<METRIC>();
            R Xt = R(0);
            // ---- stage 2 -------------------------------------------------------------------------------------
            {
                const R ha = h * N::a[1][0], hc = h * N::c[1];
#pragma unroll
                for (int q = 0; q < 4; q++) U[q] = rfma(ha, k[0][q], u[q]);
#pragma unroll
                for (int q = 0; q < 3; q++) X[q] = rfma(hc, u[1 + q], x[1 + q]);
                if constexpr (TDEP) Xt = rfma(hc, u[0], x[0]);
            }
            // [budget: rhs]
            accel<R, METRIC, SPIN, true>(X, U, MK, k[1], Xt);
            // [budget: stage sums]
            KSTORE(1);
            // ---- stage 3 -------------------------------------------------------------------------------------
            {
                const R w1 = h * N::a[2][1], w0 = h * N::a[2][0], hc = h * N::c[2], h2a = h2 * N::A2[2][0];
#pragma unroll
                for (int q = 0; q < 4; q++) U[q] = rfma(w1, KL(1, q), rfma(w0, k[0][q], u[q]));
#pragma unroll
                for (int q = 0; q < 3; q++) X[q] = rfma(h2a, k[0][1 + q], rfma(hc, u[1 + q], x[1 + q]));
                if constexpr (TDEP) Xt = rfma(h2a, k[0][0], rfma(hc, u[0], x[0]));
            }
            // [budget: rhs]
            accel<R, METRIC, SPIN, true>(X, U, MK, k[2], Xt);
            // [budget: stage sums]
            KSTORE(2);
            // ---- stages 4, 5, 6 ----------------------------------------------------------------------------------
#pragma unroll
            for (int q = 0; q < 4; q++)
                U[q] = rfma(h, rfma(N::a[3][2], KL(2, q), rfma(N::a[3][1], KL(1, q), N::a[3][0] * k[0][q])), u[q]);
#pragma unroll
            for (int q = 0; q < 3; q++)
                X[q] = rfma(h2, rfma(N::A2[3][1], KL(1, 1 + q), N::A2[3][0] * k[0][1 + q]),
                            rfma(h * N::c[3], u[1 + q], x[1 + q]));
            if constexpr (TDEP) Xt = rfma(h2, rfma(N::A2[3][1], KL(1, 0), N::A2[3][0] * k[0][0]), rfma(h * N::c[3], u[0], x[0]));
            // [budget: rhs]
            accel<R, METRIC, SPIN, true>(X, U, MK, k[3], Xt);
            // [budget: stage sums]
            KSTORE(3);
#pragma unroll
            for (int q = 0; q < 4; q++)
                U[q] = rfma(h, rfma(N::a[4][3], KL(3, q), rfma(N::a[4][2], KL(2, q), rfma(N::a[4][1], KL(1, q),
                            N::a[4][0] * k[0][q]))), u[q]);
#pragma unroll
            for (int q = 0; q < 3; q++)
                X[q] = rfma(h2, rfma(N::A2[4][2], KL(2, 1 + q), rfma(N::A2[4][1], KL(1, 1 + q), N::A2[4][0] * k[0][1 + q])),
                            rfma(h * N::c[4], u[1 + q], x[1 + q]));
            if constexpr (TDEP) Xt = rfma(h2, rfma(N::A2[4][2], KL(2, 0), rfma(N::A2[4][1], KL(1, 0), N::A2[4][0] * k[0][0])),
                                          rfma(h * N::c[4], u[0], x[0]));
            // [budget: rhs]
            accel<R, METRIC, SPIN, true>(X, U, MK, k[4], Xt);
            // [budget: stage sums]
            KSTORE(4);
#pragma unroll
            for (int q = 0; q < 4; q++)
                U[q] = rfma(h, rfma(N::a[5][4], KL(4, q), rfma(N::a[5][3], KL(3, q), rfma(N::a[5][2], KL(2, q),
                            rfma(N::a[5][1], KL(1, q), N::a[5][0] * k[0][q])))), u[q]);
#pragma unroll
            for (int q = 0; q < 3; q++)
                X[q] = rfma(h2, rfma(N::A2[5][3], KL(3, 1 + q), rfma(N::A2[5][2], KL(2, 1 + q), rfma(N::A2[5][1], KL(1, 1 + q),
                            N::A2[5][0] * k[0][1 + q]))), rfma(h * N::c[5], u[1 + q], x[1 + q]));
            if constexpr (TDEP) Xt = rfma(h2, rfma(N::A2[5][3], KL(3, 0), rfma(N::A2[5][2], KL(2, 0), rfma(N::A2[5][1], KL(1, 0),
                                          N::A2[5][0] * k[0][0]))), rfma(h * N::c[5], u[0], x[0]));
            // [budget: rhs]
            accel<R, METRIC, SPIN, true>(X, U, MK, k[5], Xt);
            // [budget: stage sums]
            KSTORE(5);
            // ---- stage 7 = the step result (FSAL) ----------------------------------------------------------------
#pragma unroll
            for (int q = 0; q < 4; q++) {
                un[q] = rfma(h, rfma(N::a[6][5], KL(5, q), rfma(N::a[6][4], KL(4, q), rfma(N::a[6][3], KL(3, q),
                             rfma(N::a[6][2], KL(2, q), rfma(N::a[6][1], KL(1, q), N::a[6][0] * k[0][q]))))), u[q]);
                xn[q] = rfma(h2, rfma(N::A2[6][4], KL(4, q), rfma(N::A2[6][3], KL(3, q), rfma(N::A2[6][2], KL(2, q),
                             rfma(N::A2[6][1], KL(1, q), N::A2[6][0] * k[0][q])))), rfma(h * N::c[6], u[q], x[q]));
            }
            // [budget: rhs]
            accel<R, METRIC, SPIN, true>(xn + 1, un, MK, k[6], xn[0]);

            // The error estimate, the controller, the reach bound and (NEAR) the sample-point scan ALSO run in uniform control
            // flow: a wave64 VALU instruction with few lanes enabled is not cheaper on this chip, it is 2.4 x DEARER — f64
            // arithmetic with <= 8 lanes in EXEC issues at 12.4 instead of 5.25 clocks, f32 with <= 16 lanes likewise
            // (tools/micro/exec_mask_rates.hip, profiles/r03/exec_mask_rates.log) — and the waves that decide when a small
            // launch ends (the last rays of the FAR pass, the long stayers of the NEAR pass) are exactly the ones with a
            // handful of live lanes.  So lanes without a ray ("ghosts") walk through this block too, on whatever state they
            // hold and h = 0; every side effect below is gated by `run`, and their decisions are wiped at the end of the block.
            // (-DRTGR_GHOST_LANES=0: the block under the running lanes' EXEC mask, for A/B.)
            if (RTGR_GHOST_LANES ? true : run) {
        // [budget: error norm]
                // ---- embedded error, residual norm in f32 ----------------------------------------
                // ũ_q = h e_q with e = (Σ b̃_l k_l, h Σ BT2_l k_l + Σb̃ u): the common factor h is applied ONCE, to the f32 sum
                // of squares (eight f64 products less per step), and the (u, x) pair of a component goes through the
                // residual arithmetic as one packed f32 operand (v_pk_mul_f32 / v_pk_fma_f32).
                float2_t acc2 = {0.0f, 0.0f};
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const R eu = rfma(N::bt[6], k[6][q], rfma(N::bt[5], KL(5, q), rfma(N::bt[4], KL(4, q),
                                     rfma(N::bt[3], KL(3, q), rfma(N::bt[2], KL(2, q), rfma(N::bt[1], KL(1, q), N::bt[0] * k[0][q]))))));
                    const R ex = rfma(h, rfma(N::BT2[5], KL(5, q), rfma(N::BT2[4], KL(4, q), rfma(N::BT2[3], KL(3, q),
                                     rfma(N::BT2[2], KL(2, q), rfma(N::BT2[1], KL(1, q), N::BT2[0] * k[0][q]))))), N::sbt * u[q]);
                    const float2_t isk = {__builtin_amdgcn_rcpf((float)rfma(rmaxabs<R>(u[q], un[q]), reltol, abstol)),
                                          __builtin_amdgcn_rcpf((float)rfma(rmaxabs<R>(x[q], xn[q]), reltol, abstol))};
                    const float2_t e = {(float)eu, (float)ex};
                    const float2_t r2 = e * isk;
                    acc2 = __builtin_elementwise_fma(r2, r2, acc2);
                }
                // EEst² — the square root is never taken: the tests are EEst <= 1 <=> EEst² <= 1, and the controller works with
                // log2 EEst = ½ log2 EEst² (sqrtf's IEEE expansion was ~15 instructions per step)
                // (the two factors of h one after the other, not as h²: (float)h squared underflows below |h| ~ 1e-19 while the sum may
                //  already be huge — 0 · inf = NaN would end the ray as RTGR_RAY_NAN instead of DTMIN, a flushed h² would ACCEPT the
                //  step with maximum growth; same three multiplies.  ADVICE r3.)
                const float hf32 = (float)h;
                const float EEst2 = ((acc2.x + acc2.y) * hf32) * (0.125f * hf32);
        // [budget: controller]
                uint32_t done = 0xffu;  // 0xff = still running, else rtgr_ray_status
                bool is_event = false, is_interior = false, handed = false, hand_back = false;
                R top = R(0);
                R cc[4][4];  // position polynomial of this step (set when the step is accepted; read only on events)
                // RTGR_GRID: every accepted step that ends outside the grid's valid box ends its ray (below), so a running ray outside
                // the box is one that STARTED there: it ends as RTGR_RAY_OUTSIDE before its first step
                bool start_outside = false;
                if constexpr (Sampled<R, METRIC>::is) start_outside = !Sampled<R, METRIC>::inside(MK, x);   // (a time-dependent grid: t too)
                if (start_outside) {
                    done = RTGR_RAY_OUTSIDE;
                } else if (EEst2 != EEst2) {
                    done = RTGR_RAY_NAN;
                } else {
                    // ---- PI controller in log2 space: q = EEst^β1 / qold^β2 / γ ----------------------
                    const float le = 0.5f * flog2(fmax1_lit<__builtin_bit_cast(uint32_t, 1e-37f)>(EEst2));  // log2 of the error estimate itself (floor 3e-19)
                    float qf = fexp2(__builtin_fmaf(beta1, le, -beta2 * lq)) * igamma;
                    qf = (EEst2 == 0.0f) ? qmax_inv : fclamp1(qf, qmax_inv, qmin_inv);
        // [budget: reach bound]
                    bool hand_over = false;
                    bool need_scan = true;  // NEAR: false when no lane of the wave can see a sign change in this step
                    // NEAR: WHICH objects some lane of the wave may see change sign in this step — bit o >> mask_shift of the mask (one
                    // bit per object up to 64 objects; beyond, one per 2, 4, … neighbours of the device list, which the groups of a long
                    // list have made neighbours in space: a bit drags in what the ray is passing anyway), all ones for the passes that
                    // do not test reach.  The scan below folds only those objects into the sample points' minima: an
                    // object whose distance provably keeps its sign in this step, for every lane that takes part, cannot move the sign of
                    // the minimum (a ray outside every object stays outside the ones it cannot reach), and the sign is all the scan reads.
                    // With example2's three objects that saves little; with a list of 64 it is the difference between 9 x 64 distances
                    // per scanned step and 9 x the one or two spheres a ray is passing (2048², 64 objects, NEAR pass
                    // 65.9 -> see there).  Same results bit for bit: FULL == FAR + NEAR is under test with long lists too.
                    unsigned long long scan_mask = ~0ull;
                    // … and, for lists beyond 64 objects (where a bit stands for 2, 4, … 2048 neighbours), the positions themselves: up to
                    // RTGR_EARLY_BUF of them in the wave's LDS (the early list's buffer, idle in this pass); more than that — or "every
                    // object" — and the scan walks the mask's blocks instead
                    uint32_t ncand = RTGR_EARLY_BUF + 1u;
                    if constexpr (MODE == MODE_FAR || MODE == MODE_NEAR) {
                        if (EEst2 <= 1.0f) {
                            // ---- can ANY object's distance change sign anywhere in this step?  |x_q(θ) − x_q| <= δ_q for all
                            // θ in [0,1] (Nyström form of the dense output, beta[l] = max|B2_l(θ)|); a plane's distance then
                            // moves by <= δ_t, a sphere's by <= Σ_q δ_q (2|X_q| + δ_q), a disk's by <= max(δ_z, δ_x + δ_y).
                            R dl[4];
#pragma unroll
                            for (int q = 0; q < 4; q++) {
                                R acc2 = N::beta[0] * rabs(k[0][q]);
#pragma unroll
                                for (int l = 1; l < 6; l++) acc2 = rfma(N::beta[l], rabs(KL(l, q)), acc2);
                                dl[q] = h * rfma(h, acc2, rabs(u[q]));
                            }
                            bool safe = true;
                            const R guard = R(1) + R(1e-6);
                            if constexpr (MODE == MODE_NEAR) {
                                // a lane INSIDE an object (ps < 0: the minimum is that object's negative distance and changes sign when
                                // the ray leaves it), or without a sign yet (ps == 0), needs every object: no selection for this wave-step
                                scan_mask = __ballot(run && !(ps > R(0))) != 0ull ? ~0ull : 0ull;
                                ncand = scan_mask != 0ull ? RTGR_EARLY_BUF + 1u : 0u;
                            }
                            // (+ an absolute floor of a few hundred ulp of the operands: a distance that is itself rounding noise must go
                            //  through the real scan)
                            auto note = [&](bool safe_o, uint32_t o) {
                                safe = safe && safe_o;
                                if constexpr (MODE == MODE_NEAR) {
                                    if (__ballot(run && !safe_o) != 0ull) {
                                        scan_mask |= 1ull << (o >> mask_shift);
                                        if (__builtin_expect(mask_shift != 0u, 0)) {
                                            if (ncand < RTGR_EARLY_BUF) early_buf[ncand] = o;   // (every lane that is here writes the same word)
                                            ncand++;
                                        }
                                    }
                                }
                            };
                            // (a lane that has ruled a whole GROUP of spheres out — see below — has ruled its members out: what the
                            //  members' own tests say for that lane, asked because another lane needs them, does not count)
                            bool group_out = false, run_out = false;
                            for_each_within_reach<R>(A.sc,
                              [&](const DevObject<R>& G, int level) -> bool {   // a group of a long list (level 0), or a run of groups (1): its bounding sphere
                                // OUTSIDE the bounding sphere now, and for the whole step (the sphere test below without the absolute
                                // value): then outside every member, by at least the same margin, for the whole step — no member's
                                // distance changes sign.  The floor keeps that margin above the rounding noise of the members' own
                                // distances (|X_g| − R_g > 64 eps (|X_g| + R_g), the noise is a few eps of |X_i| + R_i <= |X_g| + 2 R_g).
                                R lhs, rhs;
                                sphere_reach<R, false>(G, x, dl, lhs, rhs);
                                const bool out = lhs > rhs;
                                if (level != 0) { run_out = out; group_out = out; }   // (a lane that has ruled the run out has ruled its groups out)
                                else group_out = run_out || out;
                                return __ballot(run && !group_out) != 0ull;
                              },
                              [&](const DevObject<R>& ob, uint32_t o) {   // the spheres of the list: no dispatch, one batch of scalar loads each
                                R lhs, rhs;
                                sphere_reach<R, true>(ob, x, dl, lhs, rhs);
                                note(group_out || lhs > rhs, o);
                              },
                              [&](const DevObject<R>& ob, uint32_t o) {   // everything else
                                bool safe_o;
                                if (ob.kind == RTGR_PLANE) {
                                    R lhs, rhs;
                                    plane_reach<R>(ob, x, dl, lhs, rhs);
                                    safe_o = lhs > rhs;
#ifdef RTGR_USER_OBJECTS
                                } else if (ob.kind == RTGR_USER_OBJECT) {
#ifdef RTGR_USER_REACH
                                    // the source's own bound of how far its distance can move inside the box |x'_q − x_q| <= δ_q
                                    // (+ a floor of a few hundred ulp of the distance's natural scale, 1 + |d|: a distance that is
                                    //  itself rounding noise goes through the real scan, as for the built-ins)
                                    const R gd[4] = {guard * dl[0], guard * dl[1], guard * dl[2], guard * dl[3]};
                                    const R du = rtgr_user_distance<R>(ob.type, x, ob.p);
                                    const R bu = rtgr_user_reach<R>(ob.type, x, ob.p, gd);
                                    safe_o = (rabs(du) > bu + R(256) * eps * (R(1) + rabs(du)));
#else
                                    safe_o = false;   // no bound given: never provably out of reach (such units run the FULL pass)
#endif
#endif
                                } else {   // RTGR_DISK
                                    R px = x[1], py = x[2];
                                    asm volatile("" : "+v"(px), "+v"(py));  // keep the disk's root inside this branch
                                    // (a maximum of three terms moves by at most the LARGEST of their moves: |z| by δ_z, the two radial
                                    //  terms by δ_ϱ <= δ_x + δ_y — not by their sum, which round 3 charged)
                                    safe_o = (rabs(disk_distance_fast<R>(ob, px, py, x[3])) > guard * rmax(dl[3], dl[1] + dl[2]));
                                }
                                note(safe_o, o);
                              });
                            if constexpr (MODE == MODE_FAR) hand_over = run && (!safe || (ps == R(0)));
                            else {
                                need_scan = !safe || (ps == R(0));
                                safe_streak = need_scan ? 0u : safe_streak + 1u;
                            }
                        }
                        // NEAR pass: a ray stays here until it ends, also after it has left every object's reach; its
                        // wave then runs with few lanes (the longest stays are 150-370 steps), so the scan is skipped
                        // whenever NO active lane needs it — a wave-uniform decision, same results by the same bound.
                        if constexpr (MODE == MODE_NEAR) {
                            need_scan = __ballot(run && (EEst2 <= 1.0f) && need_scan) != 0ull;
                            // (the mask was formed under the EXEC of the lanes that accepted their step, the same value in each of them:
                            //  read it from one of those — a lane that rejected still holds "every object", a superset and as correct —
                            //  and make it wave-uniform for the compiler too, so that the scan's per-object branches are scalar)
                            const unsigned long long m_acc = __ballot(EEst2 <= 1.0f);
                            scan_mask = uniform64(__shfl(scan_mask, m_acc != 0ull ? (int)__builtin_ctzll(m_acc) : 0, 64));
                            ncand = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl((int)ncand, m_acc != 0ull ? (int)__builtin_ctzll(m_acc) : 0, 64));
                        }
                    }
        // [budget: hand over]
                    if (hand_over) {
                        // hand the ray, in its PRE-step state, to the NEAR pass (which redoes this step with the full scan)
                        hand_store<R>(A.hand + idx * HAND_W, x, u, k[0], t, dt, ps, lq);
                        const bool early_ray = MODE == MODE_FAR && A.early && nacc < A.near_early;
                        A.meta[idx * 3] = nacc; A.meta[idx * 3 + 1] = nrej;
                        A.meta[idx * 3 + 2] = early_ray ? META_HANDED_EARLY : META_HANDED;
                        // A ray handed over EARLY in its life is passing an object it may well miss, and then it stays in
                        // the NEAR pass for the rest of its path: in example2, 1.2 % of the rays, all handed over at
                        // steps 30-34, hold 55 % of the NEAR pass's steps.  They are listed so that the NEAR pass can
                        // start with them, packed together (collected per wave in LDS, see the end of the loop body).
                        if (early_ray) list_it = true;
                        handed = true;
        // [budget: controller]
                    } else if (EEst2 <= 1.0f) {
                        nacc++;
                        lq = fmax1(le, lq_init);  // log2(max(EEst, qoldinit))
                        const R dtnew = dt * (R)__builtin_amdgcn_rcpf(qf);
                        R tnew = t + dt;
                        // snap to λ1 within 10 ulp (OrdinaryDiffEq's fixed-tstop rule) — tested only where it can hold: λ ∈ [λ0, λ1], so
                        // |tnew − λ1| < 10 eps max(|tnew|, |λ1|) needs tnew > t1_snap (a wave-uniform constant): one compare per step
                        if (tnew > t1_snap) {
                            if (rabs(tnew - t1) < R(10) * eps * rmaxabs<R>(tnew, t1)) tnew = t1;
                        }
        // [budget: scan]
                        // ---- ContinuousCallback ----------------------------------------------------
                        // x(θ) = x + θ c1 + θ² c2 + θ³ c3 + θ⁴ c4 ;  c1 = h u,  c_m = h² Σ_l R2[l][m] k_l
                        // (FAR pass: proven above that no object's distance changes sign in this step — nothing to scan)
                        if (MODE != MODE_FAR && need_scan) {
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            cc[0][q] = h * u[q];
#pragma unroll
                            for (int m = 1; m < 4; m++)
                                cc[m][q] = h2 * rfma(N::R2[5][m], KL(5, q), rfma(N::R2[4][m], KL(4, q), rfma(N::R2[3][m], KL(3, q),
                                                rfma(N::R2[2][m], KL(2, q), rfma(N::R2[1][m], KL(1, q), N::R2[0][m] * k[0][q])))));
                        }
                        bool found = false;
                        R nextc;
                        // the objects of this step's scan: by the list of positions where there is one (NEAR, lists beyond 64 objects),
                        // else by the mask (for_each_masked_by_kind: bit tests for a list in the argument block, set bits beyond)
                        auto scan_objects = [&](auto&& fs, auto&& fo) {
                            if constexpr (MODE == MODE_NEAR) {
                                if (__builtin_expect(mask_shift != 0u && ncand <= RTGR_EARLY_BUF, 0)) {
                                    typedef const DevObject<R> __attribute__((address_space(4))) * ConstTable;
                                    const ConstTable table = (ConstTable)(unsigned long long)(A.sc.more - (uint32_t)RTGR_MAX_OBJECTS);
                                    for (uint32_t c_ = 0; c_ < ncand; c_++) {
                                        const uint32_t o = (uint32_t)__builtin_amdgcn_readfirstlane((int)early_buf[c_]);
                                        if (o < A.sc.nsph) fs(*(const DevObject<R>*)(table + o), o);
                                        else fo(*(const DevObject<R>*)(table + o), o);
                                    }
                                    return;
                                }
                            }
                            for_each_masked_by_kind<R>(A.sc, scan_mask, mask_shift, fs, fo);
                        };
                        if constexpr (NPTS10) {
                            // two blocks (θ = 1/9…5/9, then 6/9…8/9 + the end point) keep the live set inside the
                            // 256-register budget; each object's parameters are fetched once per block
                            {
                                R pos[5][4], dmin[5];
#pragma unroll
                                for (int j = 0; j < 5; j++) {
                                    const R th = R(j + 1) / R(9);
                                    dmin[j] = R(__builtin_huge_val());
#pragma unroll
                                    for (int q = 0; q < 4; q++)
                                        pos[j][q] = rfma(th, rfma(th, rfma(th, rfma(th, cc[3][q], cc[2][q]), cc[1][q]), cc[0][q]), x[q]);
                                }
                                scan_objects(
                                    [&](const DevObject<R>& ob, uint32_t) { fold_sphere<R, 5>(ob, pos, dmin); },
                                    [&](const DevObject<R>& ob, uint32_t) { fold_distances<R, 5>(ob, pos, dmin); });
#pragma unroll
                                for (int j = 0; j < 5; j++) {
                                    const bool hit = (ps * dmin[j] < R(0)) && !found;
                                    top = hit ? R(j + 1) / R(9) : top;
                                    found = found || hit;
                                }
                            }
                            {
                                R pos[4][4], dmin[4];
#pragma unroll
                                for (int j = 0; j < 3; j++) {
                                    const R th = R(j + 6) / R(9);
                                    dmin[j] = R(__builtin_huge_val());
#pragma unroll
                                    for (int q = 0; q < 4; q++)
                                        pos[j][q] = rfma(th, rfma(th, rfma(th, rfma(th, cc[3][q], cc[2][q]), cc[1][q]), cc[0][q]), x[q]);
                                }
                                dmin[3] = R(__builtin_huge_val());
#pragma unroll
                                for (int q = 0; q < 4; q++) pos[3][q] = xn[q];
                                scan_objects(
                                    [&](const DevObject<R>& ob, uint32_t) { fold_sphere<R, 4>(ob, pos, dmin); },
                                    [&](const DevObject<R>& ob, uint32_t) { fold_distances<R, 4>(ob, pos, dmin); });
                                nextc = dmin[3];
#pragma unroll
                                for (int j = 0; j < 3; j++) {
                                    const bool hit = (ps * dmin[j] < R(0)) && !found;
                                    top = hit ? R(j + 6) / R(9) : top;
                                    found = found || hit;
                                }
                            }
                        } else {
                            nextc = min_distance<R>(A.sc, xn);
                            const R dth = npts > 1 ? R(1) / R(npts - 1) : R(1);
                            for (int j = 1; j + 1 < npts; j++) {
                                const R th = R(j) * dth;
                                R xi[4];
#pragma unroll
                                for (int q = 0; q < 4; q++)
                                    xi[q] = rfma(th, rfma(th, rfma(th, rfma(th, cc[3][q], cc[2][q]), cc[1][q]), cc[0][q]), x[q]);
                                const bool hit = (ps * min_distance<R>(A.sc, xi) < R(0)) && !found;
                                top = hit ? th : top;
                                found = found || hit;
                            }
                        }
                        const bool endpoint = (ps != R(0)) && (ps * nextc <= R(0));
                        found = found && (ps != R(0)) && !endpoint;
                        if (endpoint || found) {
                            top = endpoint ? R(1) : top;
                            is_event = true;
                            is_interior = found;
                            done = RTGR_RAY_EVENT;
                        }
                        if (!is_event) ps = rsign(nextc);
                        }  // scan
        // [budget: controller]
                        if (!is_event) {
                            commit = true;
                            t = tnew;
                            dt = rmin_su(dtmax, dtnew);
                            bool outside = false;   // RTGR_GRID: the step ended outside the valid box (the scan found no event in it)
                            if constexpr (Sampled<R, METRIC>::is) outside = !Sampled<R, METRIC>::inside(MK, xn);
                            if (outside) done = RTGR_RAY_OUTSIDE;
                            else if (!(t < t1)) done = RTGR_RAY_LAMBDA1;
                            else if (nacc + nrej >= A.opt.max_steps) done = RTGR_RAY_MAXSTEPS;
                            else if (!(t + dt > t)) done = RTGR_RAY_DTMIN;
                            else if (MODE == MODE_NEAR && A.allow_handback && safe_streak >= 2u && (nacc - nacc0) >= A.handback_after) hand_back = true;
                        }
                    } else {
                        nrej++;
                        // (EEst^β1, the rejected step's factor, is formed HERE: Float64 rays reject about one step in 10⁴, and an
                        //  exp2 + a product in every step's uniform flow were two issue slots — 3.6 with the transcendental's cost — for them)
                        dt = dt * (R)__builtin_amdgcn_rcpf(fmin1(qmin_inv, fexp2(beta1 * le) * igamma));
                        if (nacc + nrej >= A.opt.max_steps) done = RTGR_RAY_MAXSTEPS;
                        else if (!(t + dt > t)) done = RTGR_RAY_DTMIN;
                    }
                }
        // [budget: records and bookkeeping]
                if (!run) {  // a ghost lane decides nothing
                    done = 0xffu; is_event = false; is_interior = false; handed = false; hand_back = false; commit = false;
                    list_it = false;
                }
                // ---- an event: hand the step's position polynomial to the resolve kernel (built from the step-START state,
                // so it has to happen before the commit below) -----------------------------------------------------------------
                const bool want_state = (A.recw == REC_TAIL_STATE);
                if (is_event) {
                    const RecRef<R> rec{A.hand + idx * HAND_W, A.rec + idx * (uint64_t)A.recw};
#pragma unroll
                    for (int q = 0; q < 4; q++) rec[REC_X + q] = x[q];
#pragma unroll
                    for (int m = 0; m < 4; m++)
#pragma unroll
                        for (int q = 0; q < 4; q++) rec[REC_C + 4 * m + q] = cc[m][q];
                    rec[REC_PS] = ps;
                    rec[REC_TOP] = top;
                    rec[REC_T] = t;
                    rec[REC_H] = h;
                    if (want_state) {  // u(θ) = u + h Σ_j b_j(θ) k_j  (all seven stages)
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            rec[REC_U + q] = u[q];
#pragma unroll
                            for (int m = 0; m < 4; m++)
                                rec[REC_CU + 4 * m + q] = h * rfma(N::r[6][m], k[6][q], rfma(N::r[5][m], KL(5, q),
                                    rfma(N::r[4][m], KL(4, q), rfma(N::r[3][m], KL(3, q), rfma(N::r[2][m], KL(2, q),
                                    rfma(N::r[1][m], KL(1, q), N::r[0][m] * k[0][q]))))));
                        }
                    }
                }
                // (the accepted step is committed AFTER this region, at the top level of the loop body)
                if (handed) state = L_FREE;
                if (hand_back) {
                    // NEAR -> next round's FAR pass: the ray has been out of every object's reach for two steps; its
                    // committed state goes back into the hand-over record and the cheaper pass carries it on
                    hand_store<R>(A.hand + idx * HAND_W, xn, un, k[6], t, dt, ps, lq);
                    A.meta[idx * 3] = nacc; A.meta[idx * 3 + 1] = nrej; A.meta[idx * 3 + 2] = META_HANDBACK;
                    if (MODE == MODE_NEAR) c_maxnear = c_maxnear > (nacc - nacc0) ? c_maxnear : (nacc - nacc0);
                    state = L_FREE;
                }
                if (done != 0xffu) {
                    if (!is_event) {
                        // ended without an event (λ1, step cap, dt underflow, NaN): the state as it stands, θ = 0
                        const RecRef<R> rec{A.hand + idx * HAND_W, A.rec + idx * (uint64_t)A.recw};
#pragma unroll
                        for (int q = 0; q < 4; q++) rec[REC_X + q] = commit ? xn[q] : x[q];
                        rec[REC_PS] = R(0);
                        rec[REC_TOP] = R(0);
                        rec[REC_T] = t;
                        rec[REC_H] = R(0);
                        if (want_state) {
#pragma unroll
                            for (int q = 0; q < 4; q++) rec[REC_U + q] = commit ? un[q] : u[q];
                        }
                    }
                    uint32_t* mt = A.meta + idx * 3;
                    mt[0] = nacc;
                    mt[1] = nrej;
                    mt[2] = done | (is_interior ? 0x100u : 0u);
                    if (MODE == MODE_NEAR) c_maxnear = c_maxnear > (nacc - nacc0) ? c_maxnear : (nacc - nacc0);
#ifdef RTGR_ROOT_STATS
                    if (MODE == MODE_NEAR && A.dbg) {  // per ray: accepted steps at hand-over, accepted steps in this pass
                        uint32_t* pr = (uint32_t*)(A.dbg + 4ull * 8192) + 2 * idx;
                        pr[0] = nacc0; pr[1] = nacc - nacc0;
                    }
#endif
                    if constexpr (MODE == MODE_FAR) {
                        // a ray ENDING in the FAR pass is rare (λ1, step cap, NaN — never an event): count it with
                        // atomics of its own and keep the four accumulator registers out of the 3-waves/SIMD kernel
                        if (A.counters) {
                            atomicAdd(&A.counters[0], 1ull);
                            atomicAdd(&A.counters[1], (unsigned long long)nacc);
                            atomicAdd(&A.counters[2], (unsigned long long)nrej);
                            atomicAdd(&A.counters[3], 6ull * (nacc + nrej) + 2ull);
                            if (done >= RTGR_RAY_MAXSTEPS) atomicAdd(&A.counters[6], 1ull);
                        }
                    } else {
                        c_rays += 1; c_acc += nacc; c_rej += nrej;
                        c_ev += is_event; c_int += is_interior; c_nf += (done >= RTGR_RAY_MAXSTEPS);
                    }
                    state = L_FREE;
                }
            }
        }
        // [budget: commit]
        // ---- commit the accepted step: the only place (besides the refill) where the ray state is assigned ------------
        // (the compiler emits this as 12 v_mov_b64 under the lanes' EXEC mask — not as 24 v_cndmask_b32 selects; checked
        //  in the ISA, tools/isa_mix.py --list mov)
        if (commit) {
#pragma unroll
            for (int q = 0; q < 4; q++) { x[q] = xn[q]; u[q] = un[q]; k0[q] = k[6][q]; }
        }
        // [budget: early list]
        // ---- FAR: early-list entries are collected in LDS and appended to the global list RTGR_EARLY_BUF/2 at a time:
        // an append with its own device atomic stalls the wave for the atomic's round trip every time ANY lane has one
        // (measured: +13 % on the whole pass when a sixth of the rays qualified)
        if constexpr (MODE == MODE_FAR) {
            const unsigned long long m_list = __ballot(list_it);
            if (m_list != 0ull) {
                if (list_it) early_buf[e_cnt + mask_rank(m_list, lane)] = (uint32_t)idx;
                e_cnt += (uint32_t)__builtin_popcountll(m_list);
                if (e_cnt > RTGR_EARLY_BUF / 2) { flush_early(A, early_buf, e_cnt, lane); e_cnt = 0; }
            }
        }
        // [budget: end]
    }
    if constexpr (MODE == MODE_FAR) {
        if (e_cnt != 0u) flush_early(A, early_buf, e_cnt, lane);
    }
#ifdef RTGR_ROOT_STATS
    if (A.dbg && lane == 0) {
        unsigned long long* d = A.dbg + 4ull * blockIdx.x;
        d[0] = dbg_t0; d[1] = wall_clock64(); d[2] = dbg_iters; d[3] = dbg_rays;
    }
#endif
    if (MODE != MODE_FAR && A.counters) {
        const unsigned long long s0 = wave_sum(c_rays), s1 = wave_sum(c_acc), s2 = wave_sum(c_rej),
                                 s4 = wave_sum(c_ev), s5 = wave_sum(c_int), s6 = wave_sum(c_nf);
        if (lane == 0) {
            atomicAdd(&A.counters[0], s0);
            atomicAdd(&A.counters[1], s1);
            atomicAdd(&A.counters[2], s2);
            atomicAdd(&A.counters[3], 6ull * (s1 + s2) + 2ull * s0);  // RHS evaluations: 6 per attempt + 2 per ray
            atomicAdd(&A.counters[4], s4);
            atomicAdd(&A.counters[5], s5);
            atomicAdd(&A.counters[6], s6);
        }
        if (MODE == MODE_NEAR) {  // diagnostics: the longest stay of any ray in the NEAR pass (accepted steps)
            unsigned long long mx = c_maxnear;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_down(mx, off, 64); mx = mx > o ? mx : o; }
            if (lane == 0) atomicMax(&A.counters[7], mx);
        }
    }
}

#undef KL
#undef KSTORE
template <class R, int METRIC, bool SPIN, bool NPTS10, int MODE>
__global__ __launch_bounds__(64, (waves_per_simd_of<R, METRIC, SPIN>(MODE)))
void integrate_kernel(const IntegrateArgs<R> A) {
    integrate_body<R, METRIC, SPIN, NPTS10, MODE, ldsk_of<R, METRIC, SPIN>(MODE)>(A);
}

// The a = 0 FAR pass once more at FOUR waves per SIMD (128 registers: 28 B/lane of scratch for KS_REF, none for KS_TRUE).
// Pays on big launches only — measured 84.5 vs 85.6 ms at 16.8 M rays, but 8.5 vs 7.3 ms at 1 M rays, where 4096
// persistent waves leave 4 rays per lane and the tail dominates; with spin (92 B/lane of scratch) it loses everywhere.
template <class R, int METRIC>
__global__ __launch_bounds__(64, 4) void integrate_far4_kernel(const IntegrateArgs<R> A) {
    integrate_body<R, METRIC, false, true, MODE_FAR>(A);
}

}  // namespace rtgr
