// hmm_scan16.inc — host side of the chunked scan for up to 16 states, included by hmm_engine.hip after its kernels: the
// launch wrapper, the typed view of a scan plan's workspace, and one set of drivers (s16_forward, s16_backward,
// s16_apply, s16_posterior) — the counterpart of hmm_scan_mid.inc's scan_* drivers for 17..64 states.

static int check_launch() { return hipGetLastError() == hipSuccess ? HMM_OK : HMM_ERR_LAUNCH; }

// One kernel launch.  Every argument becomes the kernel's declared parameter type by an implicit conversion that does
// not narrow (P{a}): nullptr, float * -> const float * and int -> long long pass, long long -> int does not compile.
// A kernel's default arguments are not part of its type, so all of them are spelled out here.
template <class... P, class... A>
static void launch(void (*kernel)(P...), dim3 grid, dim3 block, unsigned lds, hipStream_t st, const A &...a) {
    kernel<<<grid, block, lds, st>>>(P{a}...);
}

// the one place where a workspace offset becomes a typed pointer
template <class T>
static T *ws_at(const void *ws, size_t off) { return (T *)((char *)ws + off); }

// Optional per-kernel timing with HIP events on the launch stream (bench.py's roofline leg).
struct Profile {
    struct Span { int kernel; hipEvent_t a, b; };
    std::vector<Span> spans;
};
struct Timed {   // brackets one launch when a profile is attached
    Profile *pr; hipStream_t st; Profile::Span sp;
    Timed(Profile *pr_, int kernel, hipStream_t st_) : pr(pr_), st(st_) {
        if (!pr) return;
        sp.kernel = kernel;
        (void)hipEventCreate(&sp.a); (void)hipEventCreate(&sp.b);
        (void)hipEventRecord(sp.a, st);
    }
    ~Timed() {
        if (!pr) return;
        (void)hipEventRecord(sp.b, st);
        pr->spans.push_back(sp);
    }
};

// The regions of a scan plan's workspace (Plan::o_*), typed.
struct Ws16 {
    float *ops; int *exps; float *prefix; double *llpre; float *suffix; double *lsuf; float *ckpt; double *loglik;
    int *topo; float *phi; int *nexact, *flags; float *xend, *rstart; int *wtab, *wlist, *wcnt; double *dfix, *wshift;
    float *upi, *gops; int *gexps; float *gprefix; double *gllpre; float *gsuffix; double *glsuf;
#define WS16(m) m(ws_at<std::remove_pointer_t<decltype(m)>>(ws, p.o_##m))
    Ws16(const Plan &p, const void *ws)
        : WS16(ops), WS16(exps), WS16(prefix), WS16(llpre), WS16(suffix), WS16(lsuf), WS16(ckpt), WS16(loglik),
          WS16(topo), WS16(phi), WS16(nexact), WS16(flags), WS16(xend), WS16(rstart), WS16(wtab), WS16(wlist),
          WS16(wcnt), WS16(dfix), WS16(wshift), WS16(upi), WS16(gops), WS16(gexps), WS16(gprefix), WS16(gllpre),
          WS16(gsuffix), WS16(glsuf) {}
#undef WS16
};

// chunk operators of every (sequence, chunk): ops / exps
static void run_reduce(const float *A, const float *E, const Plan &p, float eps, char *ws, hipStream_t st,
                       Profile *pr, int exact_mode) {
    const Ws16 w(p, ws);
    const unsigned nb = (unsigned)((p.nchains + 3) / 4);
    const int force_dense = opt(HMM_OPT_FORCE_DENSE) == 1 ? 1 : 0;
    launch(k_topo_check, dim3(p.k), dim3(64), 0, st, A, w.topo, p.k, p.q, force_dense, exact_mode, eps, w.nexact,
           w.wcnt);
    // every (sequence, chunk) is served by exactly one of the two kernels, chosen on the
    // device from the support of its model's A; the other kernel's waves exit at once
    Timed t(pr, HMM_KERNEL_REDUCE, st);
    auto *sparse = p.q == TopoGene15::Q ? k_reduce_sparse<TopoGene15>
                   : p.q == TopoGene7::Q ? k_reduce_sparse<TopoGene7> : nullptr;
    if (sparse) {
        const dim3 nbs((unsigned)((p.nchains + 15) / 16));
        launch(sparse, nbs, dim3(256), 0, st, A, E, w.ops, w.exps, w.topo, p, eps);
        if (p.k > 1 || !HMM_RS_UNI)        // waves that straddle two models
            launch(p.q == TopoGene15::Q ? k_reduce_sparse<TopoGene15, true> : k_reduce_sparse<TopoGene7, true>, nbs,
                   dim3(256), 0, st, A, E, w.ops, w.exps, w.topo, p, eps);
    }
    // the dense kernel: every chain its own wave, unless a sparse kernel may have taken the model
    launch(k_reduce, dim3(sparse && nb > 4096u ? 4096u : nb), dim3(256), 0, st, A, E, w.ops, w.exps, w.topo, p, eps);
}

// chunk-level prefix / suffix vectors from the chunk operators.  pre_in .. ls_in (sequence-sharded
// calls): the vectors entering this time slab, in place of the start distribution and of ones.
static void run_scan(const float *pi, const Plan &p, float eps, char *ws, hipStream_t st, Profile *pr,
                     const float *pre_in = nullptr, const double *ll_in = nullptr, const float *suf_in = nullptr,
                     const double *ls_in = nullptr) {
    const Ws16 w(p, ws);
    Timed t(pr, HMM_KERNEL_SCAN, st);
    if (!(p.G > 0 && opt(HMM_OPT_SCAN2) != 0)) {
        launch(k_scan, dim3(p.NB), dim3(128), 0, st, pi, w.ops, w.exps, w.prefix, w.llpre, w.suffix, w.lsuf, w.loglik,
               w.topo, p, eps, pre_in, ll_in, suf_in, ls_in);
        return;
    }
    const dim3 gw((unsigned)(((long long)p.NB * p.G + 3) / 4));
    launch(k_scan_compose, gw, dim3(256), 0, st, w.ops, w.exps, w.gops, w.gexps, w.topo, p);
    Plan pg = p;                  // the same scan, over the group operators
    pg.C = p.G;
    launch(k_scan, dim3(p.NB), dim3(128), 0, st, pi, w.gops, w.gexps, w.gprefix, w.gllpre, w.gsuffix, w.glsuf, w.loglik,
           w.topo, pg, eps, pre_in, ll_in, suf_in, ls_in);
    launch(k_scan_inner, gw, dim3(128), 0, st, w.ops, w.exps, w.gprefix, w.gllpre, w.gsuffix, w.glsuf, w.prefix, w.llpre,
           w.suffix, w.lsuf, w.topo, p, eps);
}

static int run_reduce_scan(const float *A, const float *pi, const float *E, const Plan &p, float eps,
                           char *ws, hipStream_t st, Profile *pr = nullptr) {
    run_reduce(A, E, p, eps, ws, st, pr, opt(HMM_OPT_EXACT));
    run_scan(pi, p, eps, ws, st, pr);
    return check_launch();
}

// per-model routing as k_topo_check decided it; flags (the per-sequence verdict) are set once k_exact_select has run
static Routing routing(const Ws16 &w) { return Routing{w.topo, opt(HMM_OPT_EXACT), nullptr, nullptr}; }
static Routing routing_flagged(Routing rt, const Ws16 &w) { rt.flags = w.flags; return rt; }

static int win_margin(const Plan &p) { return (WIN_MARGIN_STEPS + p.T - 1) / p.T; }

static long long apply_waves(const Plan &p) {
    const long long per_model = (long long)p.b * p.C;
    return (long long)p.k * ((per_model + p.cpw - 1) / p.cpw);
}
static dim3 apply_grid(const Plan &p) { return dim3((unsigned)((apply_waves(p) + 3) / 4)); }

// the window kernels' grid: one wave per sequence with windows, at most 4096
static dim3 win_grid(const Plan &p) { return dim3((unsigned)((p.NB < 4096 ? p.NB : 4096) + 3) / 4); }

// the verdict per sequence from the certificate sums phi: flags, the window table and the counters
// handover: the posterior's scan plan (k_backward has left rstart) — the clamp between two chunks is weighed as well
static void s16_select(const Plan &p, const Ws16 &w, const Routing &rt, hipStream_t st, bool handover = false,
                       float eps = 0.f) {
    launch(k_exact_select, dim3(p.NB), dim3(64), 0, st, rt.topo, w.phi, p, rt.exact_mode, win_margin(p), w.flags,
           w.nexact, w.wtab, w.wlist, w.wcnt, w.exps, handover ? w.prefix : nullptr, handover ? w.rstart : nullptr, eps);
}

// ---- batch groups for the posterior pipeline.  The sparse reduce kernel is VALU-bound and the
// apply kernels are HBM-bound (measured: removing all arithmetic from them changes their time by
// 3 %), so a large batch is cut into groups and reduce(g+1) runs on a second stream underneath
// forward/backward(g).  Groups are independent sub-problems (sequences never interact); all use
// the chunk length of the whole problem, so results do not depend on the grouping.
#ifndef HMM_MAX_GROUPS
#define HMM_MAX_GROUPS 16
#endif
#define MAX_GROUPS HMM_MAX_GROUPS
#ifndef HMM_GROUP_MIN_SEQ
#define HMM_GROUP_MIN_SEQ 64
#endif
struct Groups {
    int n;                      // number of groups (1 = no pipelining)
    int T;                      // chunk length shared by all groups
    int b0[MAX_GROUPS + 1];     // group g owns sequences [b0[g], b0[g+1])
    Plan plan[MAX_GROUPS];
    size_t off[MAX_GROUPS];     // workspace offset of group g
    size_t total;
};

static int plan_groups(int k, int b, int L, int q, Groups *G) {
    Plan whole;
    int rc = make_plan(HMM_OP_POSTERIOR, k, b, L, q, &whole);
    if (rc) return rc;
    int n = 1;
    if (k == 1 && (long long)b * L >= (1ll << 24)) {
        // Measured on MI355X (b=1024, L=1e5): the kernels of the two streams do overlap, but each
        // slows down by as much as it overlaps (7.67 ms with 1 group, 7.62 / 7.80 / 7.92 with
        // 2 / 4 / 8), so the pipeline is off by default and kept as an opt-in knob.
        n = opt(HMM_OPT_GROUPS);
        if (n > b / HMM_GROUP_MIN_SEQ) n = b / HMM_GROUP_MIN_SEQ;
        if (n > MAX_GROUPS) n = MAX_GROUPS;
        if (n < 1) n = 1;
    }
    G->n = n;
    G->T = whole.T;
    size_t off = 0;
    for (int g = 0; g < n; ++g) {
        G->b0[g] = (int)((long long)b * g / n);
        G->b0[g + 1] = (int)((long long)b * (g + 1) / n);
        if ((rc = make_plan(HMM_OP_POSTERIOR, k, G->b0[g + 1] - G->b0[g], L, q, &G->plan[g], whole.T))) return rc;
        G->off[g] = off;
        off += G->plan[g].total;
    }
    G->total = off;
    return HMM_OK;
}

// two helper streams per device, created on first use and kept for the life of the process
static hipStream_t *helper_streams() {
    static hipStream_t pool[64][2];
    static bool ready[64];
    static std::mutex mu;                      // entry points may be called from several host threads
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!ready[dev]) {
        if (hipStreamCreateWithFlags(&pool[dev][0], hipStreamNonBlocking) != hipSuccess) return nullptr;
        if (hipStreamCreateWithFlags(&pool[dev][1], hipStreamNonBlocking) != hipSuccess) return nullptr;
        ready[dev] = true;
    }
    return pool[dev];
}

static int check_ws(size_t total, void *ws, size_t bytes) {
    if (!ws) return HMM_ERR_NULL_POINTER;
    if (bytes < total || ((uintptr_t)ws & 255)) return HMM_ERR_WORKSPACE;
    return HMM_OK;
}

// The clamp eps every entry point serves (include/hmm_engine.h, "The clamp eps"): the one check they all share.
// The comparisons are false for NaN.
static int check_eps(float eps) { return eps >= HMM_EPS_MIN && eps <= HMM_EPS_MAX ? HMM_OK : HMM_ERR_BAD_ARGUMENT; }

// ---- the drivers

// Log-likelihoods (-> loglik), with log alpha when asked for.  Routing.  Per model: k_topo_check.  Per sequence: there
// is no backward pass here, so the scan plan's forward kernel itself carries the clamp-born part of alpha_hat along and
// weighs it with the chunk scan's suffix vectors (forward_body's CERT); sequences whose sum is above EXACT_DELTA are
// walked whole by the serial plan.  The log-likelihood alone comes out of the chunk scan, so for it the kernel runs for
// the verdict only.
static int s16_forward(const float *A, const float *pi, const float *E, const Plan &p, float eps, float *log_alpha,
                       double *loglik, char *ws, hipStream_t st) {
    Plan px;
    int rc = make_xplan(p, &px);
    if (rc) return rc;
    if ((rc = run_reduce_scan(A, pi, E, p, eps, ws, st))) return rc;
    const Ws16 w(p, ws);
    const Routing rt = routing(w);
    const bool cert = rt.exact_mode == HMM_EXACT_AUTO;
    if (log_alpha || cert) {
        auto *kern = !log_alpha ? k_forward<false, false, false, true>
                     : cert ? k_forward<false, true, false, true> : k_forward<false, true, false>;
        launch(kern, apply_grid(p), dim3(256), 0, st, A, pi, E, w.prefix, w.llpre, nullptr, log_alpha, w.loglik,
               cert ? w.xend : nullptr, rt, p, eps, apply_waves(p), cert ? w.phi : nullptr, cert ? w.suffix : nullptr);
    }
    // Routed sequences: windows, forward half only — for the log-likelihood alone, and for log alpha, whose rows
    // after a window then move with the window's log-likelihood (k_window_shift_loga); what the windows cannot
    // settle is walked whole
    s16_select(p, w, rt, st);
    launch(log_alpha ? k_window_posterior<5> : k_window_posterior<4>, win_grid(p), dim3(256), 0, st, A, E, w.prefix,
           w.llpre, w.suffix, w.xend, nullptr, nullptr, w.loglik, log_alpha, w.wtab, w.wlist, w.wcnt, w.flags, w.dfix, p,
           eps, win_margin(p), log_alpha ? w.wshift : nullptr);
    if (log_alpha)
        launch(k_window_shift_loga, dim3(64, 64), dim3(256), 0, st, log_alpha, w.wtab, w.wlist, w.wcnt, w.flags,
               w.wshift, p);
    launch(log_alpha ? k_forward<false, true, true> : k_forward<false, false, true>, apply_grid(px), dim3(256), 0, st, A,
           pi, E, nullptr, nullptr, nullptr, log_alpha, w.loglik, nullptr, routing_flagged(rt, w), px, eps,
           apply_waves(px), nullptr, nullptr);
    launch(k_copy_loglik, dim3((p.NB + 255) / 256), dim3(256), 0, st, w.loglik, loglik, p.NB);
    return check_launch();
}

// log beta.  hmm_backward has no start distribution: the chunk scan's forward half (whose vectors weigh the
// certificate, backward_body's CERT3) starts from the uniform one.
static int s16_backward(const float *A, const float *E, const Plan &p, float eps, float *log_beta, char *ws,
                        hipStream_t st) {
    Plan px;
    int rc = make_xplan(p, &px);
    if (rc) return rc;
    const Ws16 w(p, ws);
    if (hipMemsetD32Async((hipDeviceptr_t)w.upi, __builtin_bit_cast(int, 1.0f / (float)p.q), (size_t)p.k * p.q, st) !=
        hipSuccess)
        return HMM_ERR_LAUNCH;
    if ((rc = run_reduce_scan(A, w.upi, E, p, eps, ws, st))) return rc;
    const Routing rt = routing(w);
    const bool cert = rt.exact_mode == HMM_EXACT_AUTO;
    launch(cert ? k_backward<3, false, true> : k_backward<3, false>, apply_grid(p), dim3(256), 0, st, A, E, nullptr,
           w.suffix, w.lsuf, w.loglik, log_beta, cert ? w.phi : nullptr, cert ? w.rstart : nullptr, rt, p, eps,
           apply_waves(p), cert ? w.prefix : nullptr);
    s16_select(p, w, rt, st);
    if (cert) {                                             // routed sequences: windows (k_window_logbeta), the rest whole
        launch(k_window_logbeta, win_grid(p), dim3(256), 0, st, A, E, w.prefix, w.suffix, w.lsuf, w.rstart, log_beta,
               w.wtab, w.wlist, w.wcnt, w.flags, w.wshift, p, eps, win_margin(p));
        launch(k_window_shift_logb, dim3(64, 64), dim3(256), 0, st, log_beta, w.wtab, w.wlist, w.wcnt, w.flags,
               w.wshift, p);
    }
    launch(k_backward<3, true>, apply_grid(px), dim3(256), 0, st, A, E, nullptr, nullptr, nullptr, w.loglik, log_beta,
           nullptr, nullptr, routing_flagged(rt, w), px, eps, apply_waves(px), nullptr);
    return check_launch();
}

// The apply stage of the posterior, after run_reduce_scan on the same plan: forward (checkpoints), backward (out), then
// the serial kernels for what is routed (allow_exact; not for a time slab of a sequence-sharded call).
// dec (hmm_posterior_decode; mode HMM_POST_PROB, no `out`): the same launches with the backward, window and
// whole-sequence kernels in their Decode form; DEC = ClassOut (hmm_class_posterior): the same with that policy.
template <class DEC = Decode>
static int s16_apply(const float *A, const float *pi, const float *E, const Plan &p, float eps, int mode, char *ws,
                     float *out, double *loglik, hipStream_t st, Profile *pr, bool allow_exact = true,
                     const DEC *dec = nullptr) {
    Plan px;
    int rc = make_xplan(p, &px);
    if (rc) return rc;
    const Ws16 w(p, ws);
    const long long nw = apply_waves(p);
    const Routing rt = routing(w);
    // The scan plan's forward / backward pair agrees on its own block length: checkpoints every HMM_POST_BLOCK
    // steps for the probability output (half the checkpoint traffic: k_forward 1.38 -> 1.24 ms in a one-process A/B;
    // 16 recomputed alpha_hat rows fit k_backward<0>'s register file at two waves per SIMD, the log modes' do not)
    const bool wide = HMM_POST_BLOCK != SUB && mode == HMM_POST_PROB && p.T % HMM_POST_BLOCK == 0;
    Plan pb = p;
    if (wide) pb.nsub = p.T / HMM_POST_BLOCK;
    {
        Timed t(pr, HMM_KERNEL_FORWARD, st);
        launch(wide ? k_forward<true, false, false, false, HMM_POST_BLOCK> : k_forward<true, false, false>, apply_grid(p),
               dim3(256), 0, st, A, pi, E, w.prefix, w.llpre, w.ckpt, nullptr, w.loglik, w.xend, rt, pb, eps, nw, nullptr,
               nullptr);
    }
    {
        Timed t(pr, HMM_KERNEL_BACKWARD, st);
        auto *kern = wide ? k_backward<0, false, false, HMM_POST_BLOCK>
                     : mode == HMM_POST_PROB ? k_backward<0, false>
                     : mode == HMM_POST_LOG ? k_backward<1, false> : k_backward<2, false>;
        if (dec)
            launch(wide ? k_backward_decode<HMM_POST_BLOCK, DEC> : k_backward_decode<SUB, DEC>, apply_grid(p), dim3(256), 0, st, A, E,
                   w.ckpt, w.suffix, w.phi, w.rstart, rt, pb, eps, nw, *dec);
        else
            launch(kern, apply_grid(p), dim3(256), 0, st, A, E, w.ckpt, w.suffix, w.lsuf, w.loglik, out, w.phi, w.rstart,
                   rt, pb, eps, nw, nullptr);
    }
    if (allow_exact && dec) {
        Timed t(pr, HMM_KERNEL_EXACT, st);
        s16_select(p, w, rt, st, true, eps);
        launch(k_window_decode<DEC>, win_grid(p), dim3(256), 0, st, A, E, w.prefix, w.llpre, w.suffix, w.xend, w.rstart, w.ckpt,
               w.loglik, w.wtab, w.wlist, w.wcnt, w.flags, w.dfix, p, eps, win_margin(p), *dec);
        launch(k_exact_decode<DEC>, apply_grid(px), dim3(256), 0, st, A, pi, E, w.ckpt, w.loglik, routing_flagged(rt, w), px, eps,
               apply_waves(px), *dec);
    } else if (allow_exact) {
        // the serial kernels: per model as k_topo_check decided, per sequence from the clamp-born mass the
        // backward kernel just summed; their waves exit at once when nothing is routed
        Timed t(pr, HMM_KERNEL_EXACT, st);
        s16_select(p, w, rt, st, true, eps);
        launch(mode == HMM_POST_PROB ? k_window_posterior<0>
               : mode == HMM_POST_LOG ? k_window_posterior<1> : k_window_posterior<2>,
               win_grid(p), dim3(256), 0, st, A, E, w.prefix, w.llpre, w.suffix, w.xend, w.rstart, w.ckpt, w.loglik, out,
               w.wtab, w.wlist, w.wcnt, w.flags, w.dfix, p, eps, win_margin(p), nullptr);
        if (mode != HMM_POST_PROB && mode != HMM_POST_LOG)
            launch(k_window_fixll, dim3(64, 64), dim3(256), 0, st, out, w.wlist, w.wcnt, w.flags, w.dfix, p);
        launch(mode == HMM_POST_PROB ? k_exact_posterior<0>
               : mode == HMM_POST_LOG ? k_exact_posterior<1> : k_exact_posterior<2>,
               apply_grid(px), dim3(256), 0, st, A, pi, E, w.ckpt, w.loglik, out, routing_flagged(rt, w), px, eps,
               apply_waves(px));
    }
    if (loglik) launch(k_copy_loglik, dim3((p.NB + 255) / 256), dim3(256), 0, st, w.loglik, loglik, p.NB);
    return HMM_OK;
}

// The posterior of every batch group: reduce + scan, then the apply stage.
template <class DEC = Decode>
static int s16_posterior(const float *A, const float *pi, const float *E, const Groups &G, float eps, int mode,
                         float *out, double *loglik, char *ws, hipStream_t st, Profile *pr,
                         const DEC *dec = nullptr) {
    int rc = HMM_OK;
#ifdef HMM_GROUPS_SERIAL
    hipStream_t *hs = nullptr;
#else
    hipStream_t *hs = G.n > 1 ? helper_streams() : nullptr;
#endif
    // group g on streams (s0, s1): reduce + scan on s0, the apply stage on s1
    auto group = [&](int g, hipStream_t s0, hipStream_t s1, hipEvent_t *reduced) {
        const Plan &p = G.plan[g];
        const size_t row = (size_t)G.b0[g] * p.L * p.q;
        rc = run_reduce_scan(A, pi, E + row, p, eps, ws + G.off[g], s0, pr);
        if (reduced) {
            (void)hipEventCreateWithFlags(reduced, hipEventDisableTiming);
            (void)hipEventRecord(*reduced, s0);
            if (rc == HMM_OK) (void)hipStreamWaitEvent(s1, *reduced, 0);
        }
        DEC dg = dec ? *dec : DEC();                         // this group's rows of the decoded outputs
        if (dec) dg.advance((size_t)G.b0[g] * p.L);
        if (rc == HMM_OK)
            rc = s16_apply(A, pi, E + row, p, eps, mode, ws + G.off[g], dec ? nullptr : out + row,
                           loglik ? loglik + G.b0[g] : nullptr, s1, pr, true, dec ? &dg : nullptr);
    };
    if (!hs) {
        // single group (or no helper streams available): everything in order on the caller's stream
        for (int g = 0; g < G.n && rc == HMM_OK; ++g) group(g, st, st, nullptr);
        return rc != HMM_OK ? rc : check_launch();
    }
    // fork: helper stream 0 runs reduce+scan of every group back to back, helper stream 1 runs
    // forward+backward of group g as soon as its reduce+scan is done; join back into `st`
    hipEvent_t ev_fork, ev_red[MAX_GROUPS], ev_join[2];
    (void)hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming);
    (void)hipEventRecord(ev_fork, st);
    (void)hipStreamWaitEvent(hs[0], ev_fork, 0);
    (void)hipStreamWaitEvent(hs[1], ev_fork, 0);
    int ngroups = 0;                            // groups whose event exists (all of them unless a launch failed);
    while (ngroups < G.n && rc == HMM_OK) {     // after a failure still join the helper streams and release the events
        group(ngroups, hs[0], hs[1], &ev_red[ngroups]);
        ++ngroups;
    }
    for (int i = 0; i < 2; ++i) {
        (void)hipEventCreateWithFlags(&ev_join[i], hipEventDisableTiming);
        (void)hipEventRecord(ev_join[i], hs[i]);
        (void)hipStreamWaitEvent(st, ev_join[i], 0);
        (void)hipEventDestroy(ev_join[i]);
    }
    (void)hipEventDestroy(ev_fork);
    for (int g = 0; g < ngroups; ++g) (void)hipEventDestroy(ev_red[g]);
    return rc != HMM_OK ? rc : check_launch();
}
