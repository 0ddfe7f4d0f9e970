// The batch engine of the verifier (host): GuessGenerator::process after matching (GuessGenerator.cpp:127-250) as a phase machine
// per frame slot, the launcher that turns a tick's argument lists into launches, and the lane scheduler that runs the ticks.
// Included by verify.hip inside its anonymous namespace, after every kernel header (verify_launch.h ... verify_sprint.h) and the
// workspaces, SideStreams, StreamCache and host helpers of verify.hip.

// ---------------------------------------------------------------------------------------------- the batch engine
// One Slot = one frame = GuessGenerator::process after matching (GuessGenerator.cpp:127-250): ClusterPerObject, then
// per object (ascending imgIdx) AdjacencyRansac::Ransac rounds (adjacency_ransac.cpp:234-309) until one fails. The
// recursion of the reference becomes an explicit phase machine per slot so that the slots of a batch can be
// advanced together: a TICK lets every live slot issue the kernels of its next phase into per-kernel lists, launches
// each non-empty list once (all slots in one grid), synchronizes once, and lets every slot consume its results
// (the ransac.h:95-135 bookkeeping is replayed on the host so that pow/log are libm's).
enum Phase { PH_CLUSTER, PH_CLUSTER_WAIT, PH_PREPALL, PH_PREPALL_WAIT, PH_OBJECT, PH_ROUND, PH_PREP_WAIT, PH_DRAW,
             PH_DRAW_WAIT, PH_EVAL2, PH_EVAL2_WAIT, PH_GROWTH, PH_GROWTH_WAIT, PH_SPRINT_WAIT, PH_DONE };

struct RoundState {                                       // computeModel (ransac.h:80-143) in flight
  uint64_t consumed = 0;                                  // draws used by completed getSamples calls of this round
  uint32_t it_drawn = 0, attempts_carry = 0;
  bool selection_empty = false, loop_done = false;
  int iterations = 0, n_best = -INT_MAX;
  double k = 1.0;
  uint32_t best_it = 0;
  uint64_t pos_after_stop = 0;
  uint32_t batch = 16, lookahead = 4096;   // evaluation batches: 16, 64, 256, 1024 (easy scenes stop within the first)
  uint32_t nvalid = 0, total_iters = 0;
  uint32_t it_begin = 0, want = 0, got = 0, S = 0, window_len = 0;   // the evaluation batch being drawn
  uint32_t n_def = 0;
  uint32_t s_floor = 0;                                   // grows x4 whenever a window ran out before the request was served
};

// TODHIP_SPRINT_MARGIN=n (diagnostics): the first look-ahead of a sprint, so that tests can put the stream's end -- and with it the
// kernel's stop-and-resume path -- anywhere in a frame's rounds (default 2^17 draws; it quadruples on every stop)
inline uint64_t sprint_margin0() {
  static const uint64_t v = [] { const char* e = getenv("TODHIP_SPRINT_MARGIN"); const long long x = e ? atoll(e) : 0; return x > 0 ? (uint64_t)x : (uint64_t)(1u << 17); }();
  return v;
}
struct Slot {
  VerifyWs* ws = nullptr;
  // inputs (device-resident form)
  const float* d_kp_xy = nullptr; const float* d_cloud = nullptr; DepthInput dep = {}; bool use_depth = false;
  const uint32_t* d_counts = nullptr; const todhip_dmatch* d_matches = nullptr; const float* d_mxyz = nullptr;
  todhip_rng* rng = nullptr;                              // caller's generator: set to the final state when the slot is done
  StreamCache* stream = nullptr;                          // shared with the slots that start from the same state
  uint64_t start_draws = 0, abs_pos = 0;                  // rng->draws at entry; draws consumed by the completed rounds
  // results
  std::vector<todhip_pose> poses;
  std::vector<uint32_t> inliers;
  std::vector<todhip_round_trace> traces;
  int rc = TODHIP_OK;
  // progress
  Phase ph = PH_DONE;
  std::vector<ObjSpan> objs;
  size_t oi = 0;
  ObjJob job = {};
  bool pending_invalidate = false;
  bool in_flight = false;                                 // its current tick runs on a side stream (run_ticks)
  // window-size hint for the next object's first draw window: what the previous objects of this frame consumed when their
  // getSamples gave up (1000 failing attempts, ~4-9k draws). Frames with many stray matches hold runs of such objects; a
  // first window sized for a healthy object (576) made each of them crawl through three windows = three ticks
  uint32_t s_hint = 0;
  std::vector<size_t> sprint_members;                      // indices into objs of the sprint in flight (sprint_kernel)
  uint64_t sprint_margin = sprint_margin0();               // rand() words the device copy of the stream reaches beyond the sprint's start
  todhip_round_trace tr = {};
  RoundState r;
};

struct Launches {
  std::vector<CopyArgs> copy_in, zero, copy_out;
  std::vector<InvArgs> inval, inval_after; std::vector<JobArgs> finite; std::vector<AdjArgs> adj; std::vector<PrepArgs> prep, prep_after;   // *_after: behind the growth kernels
  std::vector<DrawArgs> draw[DRAW_FORMS]; std::vector<ChainArgs> chain;   // one draw list per form of the kernel (draw_form_of)
  // the rnd pointers of the draw lists are resolved at launch time: a later slot of the same tick may grow (move)
  // the shared stream buffer
  std::vector<std::pair<StreamCache*, uint64_t>> draw_src[DRAW_FORMS]; std::vector<EvalArgs> eval_small, eval_big, eval_direct;
  std::vector<GrowthArgs> growth;
  std::vector<SprintArgs> sprint; std::vector<StreamCache*> sprint_src;
  std::vector<ClusterArgs> cluster; std::vector<ClusterRescaledArgs> cluster_rescaled; std::vector<PrepSmallArgs> prep_small;
};

struct Engine {
  todhip_ctx* ctx;
  hipStream_t st;
  uint32_t nq, H, Wimg, k, n_objs;
  const float* spans;
  const todhip_verify_params* prm;
  Launches L;
  size_t lane_now = 0;                                      // the lane launch_all is filling (its staging pair)

  // ==== the per-slot phase machine: issue / consume / replay / round_done, sprint issue and consume
  static SlotCtl* ctl(const Slot& s) { return s.ws->small.as<SlotCtl>(); }       // the slot's control block (device)
  static SlotMail* mail(const Slot& s) { return s.ws->m_small.as<SlotMail>(); }  // and where the host reads it
  // zero fill of the bytes [from, to) of the control block: offsetof / sizeof of the members it covers
  static CopyArgs zero_ctl(SlotCtl* c, size_t from, size_t to) {
    return {nullptr, reinterpret_cast<uint32_t*>(c) + from / sizeof(uint32_t), (uint32_t)((to - from) / sizeof(uint32_t))};
  }
  void export_small(Slot& s) {
    L.copy_out.push_back({s.ws->small.as<uint32_t>(), s.ws->m_small.as<uint32_t>(), (uint32_t)(sizeof(SlotCtl) / sizeof(uint32_t))});
  }
  void fail(Slot& s, int rc) { s.rc = rc; s.ph = PH_DONE; }
#define SLOT_HIP(expr) do { if ((expr) != hipSuccess) { fail(s, TODHIP_EHIP); return; } } while (0)

  static ObjJob make_job(const Slot& s, const ObjSpan& o) {
    VerifyWs* ws = s.ws;
    ObjJob job;
    const uint32_t n = o.n, W = (n + 63u) / 64u;
    job.n = n; job.W = W;
    job.train = ws->train.as<float>() + 3 * (size_t)o.offset; job.query = ws->query.as<float>() + 3 * (size_t)o.offset;
    job.qidx = ws->qidx.as<uint32_t>() + o.offset; job.kpxy = ws->kpxy.as<float>() + 2 * (size_t)o.offset;
    job.phys = ws->phys.as<u64>() + o.adj_off; job.samp = ws->samp.as<u64>() + o.adj_off;
    u64* bits = ws->bits.as<u64>() + o.bits_off;            // finite | valid | deg7 | inl | rest | extra | scratch
    job.finite = bits; job.valid = bits + W; job.deg7 = bits + 2 * W;
    job.sampdeg = ws->sampdeg.as<uint32_t>() + o.deg_off;
    return job;
  }
  u64* obj_bits(const Slot& s) const { return s.ws->bits.as<u64>() + s.objs[s.oi].bits_off; }

  // the trace of the round of object `obj` that starts at the stream position the completed rounds have reached
  void begin_trace(Slot& s, uint32_t obj) {
    s.tr = todhip_round_trace();
    s.tr.object = obj; s.tr.draws_before = s.start_draws + s.abs_pos; s.tr.best_count = -INT_MAX;
  }
  // the first round of object o = s.objs[s.oi], from the statistics of the all-objects preparation: -> PH_DRAW, or the host decides
  // it without a kernel (fewer than 3 valid matches, or triangle-free) and round_done has moved on to the next object
  void first_round(Slot& s, const ObjSpan& o) {
    s.job = make_job(s, o);
    ctx->counters.last_objects_verified += 1;
    s.pending_invalidate = false;
    begin_trace(s, o.obj);
    start_round(s, o.nvalid, o.degsum, o.triangle);
  }

  // one AdjacencyRansac::Ransac call starts with |valid| known (adjacency_ransac.cpp:234-241)
  void start_round(Slot& s, uint32_t nvalid, uint32_t degsum, uint32_t triangle) {
    VerifyWs* ws = s.ws;
    RoundState& r = s.r;
    TOD_DBG2("round: n=%u W=%u nvalid=%u edges=%u triangle=%u", s.job.n, s.job.W, nvalid, degsum / 2u, triangle);
    if (nvalid < 3) { round_done(s, false); return; }      // :238-241
    if (!triangle) {
      // no three mutually sample-adjacent valid matches: getSamples fails 1000 times, each attempt consuming exactly
      // |valid| + |E| draws whatever their values (round_prep_kernel), selection.empty() ends computeModel at
      // iterations_ == 0 (ransac.h:100-101) and Ransac returns nothing. No kernel, no tick.
      r = RoundState();
      s.abs_pos += (uint64_t)kMaxSampleChecks * ((uint64_t)nvalid + degsum / 2u);
      s.tr.iterations = 0; s.tr.best_iteration = 0; s.tr.best_count = -INT_MAX;
      round_done(s, false);
      return;
    }
    r = RoundState();
    r.s_floor = s.s_hint;
    r.nvalid = nvalid;
    // First evaluation batch: an object with many valid matches is expensive to evaluate (its clique gate walks a graph of
    // about that many vertices, one wave per hypothesis, and a tick lasts as long as its slowest hypothesis), and when it is
    // real its first hypotheses end the loop: with w = consensus / valid, k = log(0.01) / log(1 - w^3) (ransac.h:123-130) is
    // <= 2 from w = 0.966 on (<= 1 only from 0.9967 on). So two hypotheses, not 16; the replay asks for more if k says so.
    // Small objects keep the batch of 16 (cheap evaluations, usually needing many).
    if (nvalid >= 64u) r.batch = 2;
    r.total_iters = prm->n_ransac_iterations + 1u;          // iterations_ runs 0 .. max_iterations (ransac.h:132-134)
    SLOT_HIP(ws->iter_samples.reserve((size_t)(r.total_iters + 1) * 3 * sizeof(uint32_t)));
    SLOT_HIP(ws->gate_m.reserve((size_t)(r.total_iters + 1) * sizeof(uint32_t)));
    SLOT_HIP(ws->deferred.reserve((size_t)(r.total_iters + 1) * sizeof(uint32_t)));
    SLOT_HIP(ws->m_counts.reserve((size_t)(r.total_iters + 1) * sizeof(int32_t)));
    SLOT_HIP(ws->m_pos.reserve((size_t)(r.total_iters + 1) * sizeof(uint32_t)));
    begin_batch(s);
  }

  // the evaluation of iterations [it_lo, it_hi) (first pass), or of the deferred ones (second pass: graphs that need the whole
  // LDS of a CU, or global scratch). zero_status: first evaluation launch of the batch (the deferred list and the counters
  // accumulate over the windows of one batch)
  void push_eval(Slot& s, bool second, uint32_t it_lo, uint32_t it_hi, const uint32_t* n_items_dev, bool zero_status) {
    VerifyWs* ws = s.ws;
    RoundState& r = s.r;
    SLOT_HIP(ws->stacks.reserve((size_t)std::max(std::max(it_hi - it_lo, r.n_def), 64u) * kStackCap * sizeof(uint16_t)));
    EvalArgs A = eval_args(s.job, ws, ws->m_counts.as<int32_t>(), it_lo, it_hi, eval_lds_small(s.job.n));
    A.n_items_dev = n_items_dev;
    if (second) {
      SLOT_HIP(ws->adjc_scratch.reserve((size_t)r.n_def * kAdjcScratchWords * sizeof(u64)));
      A.lds_bytes = kEvalLdsBig; A.from_deferred = 1u; A.n_deferred = r.n_def; A.adjc_scratch = ws->adjc_scratch.as<u64>();
      L.zero.push_back(zero_ctl(ctl(s), offsetof(SlotCtl, eval_work), offsetof(SlotCtl, eval_work) + sizeof(uint32_t)));
      L.eval_big.push_back(A);
      return;
    }
    if (zero_status) L.zero.push_back(zero_ctl(ctl(s), offsetof(SlotCtl, eval_work), offsetof(SlotCtl, eval) + sizeof(EvalStatus)));   // the work counter .. the status
    // A few hypotheses of an object whose consensus lists (about all of its valid matches when the object is really there)
    // will not fit the 48 KB carve: straight to a whole CU's LDS instead of a first pass that only finds that out
    if (it_hi - it_lo <= 16u && gate_lds_bytes(r.nvalid) + 4096u > kEvalLdsSmall) {
      A.lds_bytes = kEvalLdsBig;
      L.eval_direct.push_back(A);
    } else {
      L.eval_small.push_back(A);
    }
  }

  // ---- issue: queue the kernels of the slot's next phase
  void issue(Slot& s) {
    VerifyWs* ws = s.ws;
    SlotCtl* const c = ctl(s);
    if (s.ph == PH_CLUSTER) {                               // ClusterPerObject, one launch (cluster_frame_kernel)
      ClusterArgs ca;
      ca.kp_xy = s.d_kp_xy; ca.cloud = s.use_depth ? nullptr : s.d_cloud; ca.depth = s.dep.d_depth; ca.counts = s.d_counts;
      ca.matches = s.d_matches; ca.mxyz = s.d_mxyz; ca.nq = nq; ca.k = k; ca.H = H; ca.Wimg = Wimg; ca.n_objs = n_objs; ca.qidx_add = 0u;
      ca.depth_is_u16 = s.dep.is_u16; ca.fx = s.dep.fx; ca.fy = s.dep.fy; ca.cx = s.dep.cx; ca.cy = s.dep.cy;
      cluster_scratch(ca, ws);
      ca.hist = ws->c_hist.as<uint32_t>(); ca.goff = ws->c_goff.as<uint32_t>();
      ca.train = ws->train.as<float>(); ca.qidx = ws->qidx.as<uint32_t>(); ca.m_ctl = &mail(s)->tail.cluster;
      if (s.use_depth && s.dep.rescale) L.cluster_rescaled.push_back({ca, s.dep.geom});   // depth at its own size: looked up through the geometry
      else L.cluster.push_back(ca);
      s.ph = PH_CLUSTER_WAIT;
      return;
    }
    if (s.ph == PH_PREPALL) {
      // FillAdjacency and the first round's validity/degree pass of EVERY object of the frame in this one tick: they
      // do not depend on the rand() stream, and an object with < 3 valid matches then costs no tick at all
      L.zero.push_back({nullptr, ws->nvalid.as<uint32_t>(), 4u * (uint32_t)std::max<size_t>(s.objs.size(), 1)});
      for (size_t i = 0; i < s.objs.size(); ++i) {
        if (s.objs[i].n < 3) continue;
        const ObjJob job = make_job(s, s.objs[i]);
        if (job.n <= 64u) {                                  // finite + adjacency + statistics by one wave
          PrepSmallArgs pa;
          pa.job = job; pa.stats = ws->nvalid.as<uint32_t>() + 4 * i; pa.span = spans[s.objs[i].obj]; pa.err = prm->sensor_error;
          L.prep_small.push_back(pa);
          continue;
        }
        L.finite.push_back({job});
        L.adj.push_back({job, spans[s.objs[i].obj], prm->sensor_error});
        L.prep.push_back({job, ws->nvalid.as<uint32_t>() + 4 * i, nullptr, 0u});
      }
      L.copy_out.push_back({ws->nvalid.as<uint32_t>(), ws->m_nvalid.as<uint32_t>(), 4u * (uint32_t)std::max<size_t>(s.objs.size(), 1)});
      s.ph = PH_PREPALL_WAIT;
      return;
    }
    while (s.ph == PH_OBJECT) {
      // Ransac returns no inliers for < 3 valid matches and draws nothing (:238-241)
      while (s.oi < s.objs.size() && s.objs[s.oi].n < 3) ++s.oi;
      if (s.oi >= s.objs.size()) { s.ph = PH_DONE; return; }
      if (sprint_on() && sprint_live(s.objs[s.oi])) { issue_sprint(s); return; }
      first_round(s, s.objs[s.oi]);                         // -> PH_DRAW, or straight on to the next object
    }
    if (s.ph == PH_ROUND) {                                 // one AdjacencyRansac::Ransac call (GuessGenerator.cpp:192-231)
      if (s.pending_invalidate) {
        L.inval.push_back({s.job, ws->kp_bits.as<u64>(), obj_bits(s) + 6 * s.job.W, nullptr, 0u});
        s.pending_invalidate = false;
      }
      L.zero.push_back(zero_ctl(c, 0, sizeof(SlotCtl)));
      L.prep.push_back({s.job, c->prep, nullptr, 0u});
      export_small(s);
      begin_trace(s, s.objs[s.oi].obj);
      s.ph = PH_PREP_WAIT;
      return;
    }
    if (s.ph == PH_DRAW) {
      RoundState& r = s.r;
      // window = stream positions the requested iterations are expected to consume: 4 per iteration for a start
      // (3 draws + the odd failed attempt), then 1.5 x what this round's iterations consumed so far -- objects without
      // a consistent subset burn hundreds of draws per iteration in failed attempts, and a window sized for 4 made
      // them crawl through dozens of ticks
      const uint64_t seen_it = (uint64_t)r.it_begin + r.got;
      const uint64_t per_it = seen_it ? std::max<uint64_t>(4u, (3u * r.consumed / seen_it + 1u) / 2u + 1u) : 4u;
      r.S = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(per_it * (r.want - r.got) + 512u, r.s_floor), 1u << 20);
      r.window_len = r.S + r.lookahead;
      SLOT_HIP(s.stream->ensure_device(s.abs_pos + r.consumed + r.window_len, st));
      SLOT_HIP(ws->table.reserve((size_t)r.S * sizeof(DrawEntry)));
      const DrawForm form = draw_form_of(s.job.W);         // one lane per position up to 512 matches, one wave beyond
      L.draw[form].push_back({s.job, nullptr, r.window_len, r.S, ws->table.as<DrawEntry>()});
      L.draw_src[form].push_back({s.stream, s.abs_pos + r.consumed});
      ChainArgs ca = {ws->table.as<DrawEntry>(), r.S, r.want - r.got, r.attempts_carry, r.it_begin + r.got,
                      ws->iter_samples.as<uint32_t>(), ws->m_pos.as<uint32_t>(), &c->chain};
      L.chain.push_back(ca);
      // the evaluation of the iterations this walk draws rides in the same tick: its grid covers everything still wanted, and
      // the kernel takes the number that really exist from the walk's ChainOut. One host round trip less per evaluation batch.
      push_eval(s, false, r.it_begin + r.got, r.it_begin + r.want, &c->chain.n_done, r.got == 0u);
      export_small(s);
      s.ph = PH_DRAW_WAIT;
      return;
    }
    if (s.ph == PH_EVAL2) {
      push_eval(s, true, 0u, 0u, nullptr, true);
      export_small(s);
      s.ph = PH_EVAL2_WAIT;
      return;
    }
    if (s.ph == PH_GROWTH) {                                // growth (adjacency_ransac.cpp:255-308)
      const uint32_t kp_words = (nq + 63u) / 64u, W = s.job.W;
      u64* d_bits = obj_bits(s);
      GrowthArgs ga = {s.job, ws->iter_samples.as<uint32_t>() + 3 * (size_t)s.r.best_it, prm->sensor_error, d_bits + 3 * W,
                       d_bits + 4 * W, d_bits + 5 * W, ws->m_kp.as<uint32_t>(), ws->kp_bits.as<u64>(), kp_words,
                       &c->growth};
      L.growth.push_back(ga);
      // If the pose is accepted (enough inlier keypoints, GuessGenerator.cpp:205-206) the object gets another round, which starts
      // with InvalidateQueryIndices and the validity / degree pass: both ride in this tick behind the growth, gated on the device
      // by the count the growth kernel writes, so an accepted pose costs no tick of its own. (Not accepted: they do nothing.)
      const uint32_t* gate = &c->growth.n_kp_inliers;
      L.zero.push_back(zero_ctl(c, 0, offsetof(SlotCtl, growth)));   // everything in front of GrowthOut, prep (the pass's counters) included
      L.inval_after.push_back({s.job, ws->kp_bits.as<u64>(), obj_bits(s) + 6 * s.job.W, gate, prm->min_inliers});
      L.prep_after.push_back({s.job, c->prep, gate, prm->min_inliers});
      export_small(s);
      s.ph = PH_GROWTH_WAIT;
      return;
    }
  }

  // ---- sprint_kernel: the live objects of at most kSprintN matches from s.oi up to the next live big object, in one launch
  static bool sprint_on() {
    static const bool on = [] { const char* e = getenv("TODHIP_VERIFY_SPRINT"); return !(e && e[0] == '0'); }();   // read once
    return on;
  }
  static bool sprint_live(const ObjSpan& o) {
    return o.n >= 3u && o.n <= kSprintN && (o.resume || (o.nvalid >= 3u && o.triangle != 0u));
  }
  void issue_sprint(Slot& s) {
    VerifyWs* ws = s.ws;
    SLOT_HIP(ws->m_sprint.reserve(kSprintMaxObjs * sizeof(SprintObj)));
    SLOT_HIP(ws->m_sprint_out.reserve((kSprintHdrWords + (size_t)kSprintMaxRecs * kSprintRecWords) * sizeof(uint32_t)));
    SLOT_HIP(ws->m_sprint_kp.reserve((size_t)kSprintMaxRecs * kSprintN * sizeof(uint32_t)));
    SLOT_HIP(ws->sprint_status.reserve(16 * sizeof(uint32_t)));
    SLOT_HIP(ws->sprint_stack.reserve((size_t)kSprintWaves * kSprintStackCap * sizeof(uint16_t)));
    SprintObj* list = ws->m_sprint.as<SprintObj>();
    s.sprint_members.clear();
    uint64_t skip = 0, total_skip = 0;
    for (size_t i = s.oi; i < s.objs.size() && s.sprint_members.size() < kSprintMaxObjs; ++i) {
      const ObjSpan& o = s.objs[i];
      if (o.n < 3u) continue;
      if (sprint_live(o)) {
        SprintObj so;
        so.job = make_job(s, o); so.skip = skip; so.index = (uint32_t)i; so.pad = 0;
        list[s.sprint_members.size()] = so;
        s.sprint_members.push_back(i);
        total_skip += skip; skip = 0;
        continue;
      }
      if (o.nvalid < 3u) continue;                           // no round, no draw (:238-241)
      if (o.triangle) break;                                 // a live big object: the sprint ends before it
      skip += (uint64_t)kMaxSampleChecks * ((uint64_t)o.nvalid + o.degsum / 2u);   // triangle-free: start_round
    }
    SLOT_HIP(s.stream->ensure_device(s.abs_pos + total_skip + s.sprint_margin, st));
    SprintArgs a;
    a.objs = list; a.rnd = nullptr; a.rnd_len = 0; a.pos0 = s.abs_pos; a.kceil = tod_ws<VerifyPool>(ctx)->kceil.as<uint32_t>();
    a.out = ws->m_sprint_out.as<uint32_t>(); a.kp_out = ws->m_sprint_kp.as<uint32_t>();
    a.status = ws->sprint_status.as<EvalStatus>(); a.stack = ws->sprint_stack.as<uint16_t>();
    a.n_objs = (uint32_t)s.sprint_members.size(); a.max_iterations = prm->n_ransac_iterations; a.min_inliers = prm->min_inliers;
    a.err = prm->sensor_error; a.rec_cap = kSprintMaxRecs; a.kp_cap = kSprintMaxRecs * kSprintN;
    SprintHeader* hdr = ws->m_sprint_out.as<SprintHeader>();
    hdr->n_rec = 0u; hdr->reason = SPRINT_ERROR; hdr->n_done = 0u;   // (overwritten by the kernel)
    L.zero.push_back({nullptr, reinterpret_cast<uint32_t*>(a.status), (uint32_t)(sizeof(EvalStatus) / sizeof(uint32_t))});
    L.sprint.push_back(a);
    L.sprint_src.push_back(s.stream);                        // rnd / rnd_len are resolved at launch time (the shared stream may move)
    s.ph = PH_SPRINT_WAIT;
  }
  void consume_sprint(Slot& s) {
    VerifyWs* ws = s.ws;
    const SprintHeader& hdr = *ws->m_sprint_out.as<SprintHeader>();
    const SprintRecord* recs = sprint_records(ws->m_sprint_out.as<uint32_t>());
    const uint32_t* kp_out = ws->m_sprint_kp.as<uint32_t>();
    const uint32_t n_rec = hdr.n_rec, reason = hdr.reason, n_done = hdr.n_done;
    TOD_DBG("sprint: %zu objects, %u done, %u records, reason %u, gate calls %u, hypotheses %u, windows %u; ticks: ring %u attempt %u walk %u eval %u "
            "book %u growth %u all %u", s.sprint_members.size(), n_done, n_rec, reason, hdr.gate_calls, hdr.hypotheses, hdr.n_windows, hdr.t_ring, hdr.t_att,
            hdr.t_walk, hdr.t_eval, hdr.t_book, hdr.t_grow, hdr.t_all);
    if (reason == SPRINT_ERROR || n_rec > kSprintMaxRecs || n_done > s.sprint_members.size()) {
      if (tod_debug()) fprintf(stderr, "[todhip] sprint error: detail %u status %u\n", hdr.err_detail, hdr.reason);
      fail(s, TODHIP_ESCRATCH);
      return;
    }
    ctx->counters.last_gate_calls += hdr.gate_calls;
    ctx->counters.last_hypotheses += hdr.hypotheses;
    ctx->counters.last_sprint_launches += 1;
    ctx->counters.last_sprint_rounds += n_rec;
    uint32_t ri = 0;
    for (uint32_t m = 0; m < s.sprint_members.size(); ++m) {
      const size_t idx = s.sprint_members[m];
      const bool complete = m < n_done;
      const bool touched = complete || (ri < n_rec && recs[ri].obj == m);
      if (!touched) break;                                   // the wave stopped before this object: PH_OBJECT takes it from here
      // the objects the host decides without a kernel on the way (first round: fewer than 3 valid matches, or triangle-free)
      while (s.oi < idx) {
        if (s.objs[s.oi].n < 3u) { ++s.oi; continue; }
        first_round(s, s.objs[s.oi]);                        // -> round_done: ++s.oi
        if (s.ph == PH_DONE) return;                         // (a failure)
      }
      ObjSpan& o = s.objs[idx];
      if (!o.counted) { ctx->counters.last_objects_verified += 1; o.counted = true; }
      for (; ri < n_rec; ++ri) {
        const SprintRecord& rec = recs[ri];
        if (rec.obj != m) break;
        const uint64_t consumed = ((uint64_t)rec.consumed_hi << 32) | rec.consumed_lo;
        begin_trace(s, o.obj);
        s.tr.iterations = rec.iterations; s.tr.best_iteration = rec.best_it; s.tr.best_count = rec.n_best;
        s.abs_pos += consumed;
        const uint32_t n_kp = rec.grew ? rec.n_kp : 0u;
        if (close_round(s, n_kp)) {
          if (rec.kp_offset + n_kp > kSprintMaxRecs * kSprintN) { fail(s, TODHIP_ESCRATCH); return; }
          push_pose(s, o.obj, rec.R, rec.T, kp_out + rec.kp_offset, n_kp);
        }
      }
      if (!complete) {                                       // relaunch from this object; the kernel recomputes its statistics
        o.resume = true;
        s.oi = idx;
        break;
      }
      s.oi = idx + 1;
    }
    if (reason == SPRINT_NEED_STREAM) {
      if (s.sprint_margin >= (1ull << 28)) { fail(s, TODHIP_ESCRATCH); return; }
      s.sprint_margin *= 4u;
    }
    s.sprint_members.clear();
    s.ph = PH_OBJECT;
  }

  // ---- one evaluation batch of computeModel starts: draw `want` iterations (as many windows as it takes)
  void begin_batch(Slot& s) {
    RoundState& r = s.r;
    r.it_begin = r.it_drawn;
    r.want = std::min(r.batch, r.total_iters - r.it_begin);
    r.got = 0;
    if (r.got < r.want && !r.selection_empty) s.ph = PH_DRAW; else after_draw(s);
  }
  void after_draw(Slot& s) {
    RoundState& r = s.r;
    r.it_drawn = r.it_begin + r.got;
    if (r.got > 0) eval_done(s, false); else replay(s);    // the iterations were evaluated in the ticks that drew them
  }
  // the first evaluation pass of a batch is complete (its status words are in the mailbox), or the second one
  void eval_done(Slot& s, bool second) {
    RoundState& r = s.r;
    const EvalStatus& es = mail(s)->eval;
    if (!second) {
      ctx->counters.last_gate_calls += es.gate_calls;
      r.n_def = es.n_deferred;
      TOD_DBG2("  eval done: gate calls=%u deferred=%u", es.gate_calls, r.n_def);
      if (r.n_def > 0) { s.ph = PH_EVAL2; return; }
    }
    ctx->counters.last_hypotheses += r.got;
    replay(s);
  }
  bool eval_failed(Slot& s) {
    const EvalStatus& es = mail(s)->eval;
    if (es.error == 0) return false;
    if (tod_debug())
      fprintf(stderr, "[todhip] eval status %u: g=%u value=%u m=%u it=%u (n=%u W=%u)\n", es.error, es.detail_g, es.detail_value, es.detail_m,
              es.detail_it, s.job.n, s.job.W);
    fail(s, TODHIP_ESCRATCH);
    return true;
  }
  // ---- ransac.h:95-135 over the iterations known so far
  void replay(Slot& s) {
    RoundState& r = s.r;
    const int32_t* hc = s.ws->m_counts.as<int32_t>();
    const uint32_t* hp = s.ws->m_pos.as<uint32_t>();
    while (!r.loop_done) {
      if (!(r.iterations < r.k)) { r.loop_done = true; r.pos_after_stop = r.iterations > 0 ? hp[r.iterations - 1] : 0; break; }
      if ((uint32_t)r.iterations >= r.it_drawn) {
        if (r.selection_empty) { r.loop_done = true; r.pos_after_stop = r.consumed; }   // selection.empty() -> break (:100-101)
        break;                                              // need more iterations
      }
      const int n_count = hc[r.iterations];
      if (n_count > r.n_best) {
        r.n_best = n_count;
        r.best_it = (uint32_t)r.iterations;
        r.k = ransac_k((double)r.n_best / (double)r.nvalid);
      }
      ++r.iterations;
      if (r.iterations > (int)prm->n_ransac_iterations) { r.loop_done = true; r.pos_after_stop = hp[r.iterations - 1]; }
    }
    // next batch = what the loop still needs given the best model so far (k of :130): a hopeless object (k >> the
    // iteration budget) gets all of its remaining iterations evaluated at once instead of in 16/64/256/1024 steps
    {
      const double need = r.k - (double)r.iterations;
      const uint32_t want = need >= (double)kMaxEvalWaves ? kMaxEvalWaves : (uint32_t)std::max(1.0, std::ceil(need));
      r.batch = std::max(std::min<uint32_t>(r.batch * 4u, kMaxEvalWaves), std::min(want, kMaxEvalWaves));
    }
    if (!r.loop_done) { begin_batch(s); return; }
    // advance the caller's generator by exactly the draws the reference would have consumed
    s.abs_pos += r.pos_after_stop;
    s.tr.iterations = (uint32_t)r.iterations; s.tr.best_iteration = r.best_it; s.tr.best_count = r.n_best;
    if (r.n_best <= 0) { round_done(s, false); return; }   // inliers_.empty(): computeModel() == false (:137-138)
    s.ph = PH_GROWTH;
  }
  // a round is over, s.abs_pos behind its draws: the tail of its trace; whether its pose is accepted (GuessGenerator.cpp:205-206)
  bool close_round(Slot& s, uint32_t n_kp) {
    ctx->counters.last_rounds += 1;
    s.tr.draws_after = s.start_draws + s.abs_pos; s.tr.n_inlier_kp = n_kp; s.tr.accepted = n_kp >= prm->min_inliers;
    s.traces.push_back(s.tr);
    return n_kp >= prm->min_inliers;
  }
  // an accepted pose (GuessGenerator.cpp:207-230): R (9 floats), t (3) and the n_kp inlier keypoints from where the round left them
  void push_pose(Slot& s, uint32_t obj, const void* R, const void* t, const uint32_t* kp, uint32_t n_kp) {
    todhip_pose p;
    std::memset(&p, 0, sizeof(p));
    p.object = obj;
    std::memcpy(p.R, R, sizeof(p.R));
    std::memcpy(p.t, t, sizeof(p.t));
    p.inlier_begin = (uint32_t)s.inliers.size();
    s.inliers.insert(s.inliers.end(), kp, kp + n_kp);
    p.inlier_end = (uint32_t)s.inliers.size();
    s.poses.push_back(p);
    ctx->counters.last_poses += 1;
  }
  void round_done(Slot& s, bool have_pose) {
    const SlotMail* m = mail(s);
    const GrowthOut* go = &m->growth;
    const uint32_t n_kp = have_pose ? go->n_kp_inliers : 0u;
    if (!close_round(s, n_kp)) { ++s.oi; s.ph = PH_OBJECT; return; }
    push_pose(s, s.objs[s.oi].obj, go->R, go->T, s.ws->m_kp.as<uint32_t>(), n_kp);
    // InvalidateQueryIndices and the next round's validity pass (:207-230) ran behind the growth kernel in this tick
    s.pending_invalidate = false;
    begin_trace(s, s.objs[s.oi].obj);
    start_round(s, m->prep[0], m->prep[1], m->prep[2]);
  }

  // ---- consume: the tick's results are in the mailbox
  void consume(Slot& s) {
    VerifyWs* ws = s.ws;
    const SlotMail* m = mail(s);
    RoundState& r = s.r;
    if (s.ph == PH_CLUSTER_WAIT) {
      if (m->tail.cluster.error != 0) { fail(s, TODHIP_ERANGE); return; }
      if (m->tail.cluster.n_kept == 0) { s.ph = PH_DONE; return; }   // n_all: no match kept
      const uint32_t* hist = ws->m_hist.as<uint32_t>();
      uint32_t total = 0, max_n = 0;
      s.objs.clear();
      for (uint32_t o = 0; o < n_objs; ++o) {
        if (hist[o]) s.objs.push_back({o, total, hist[o]});
        total += hist[o];
        max_n = std::max(max_n, hist[o]);
      }
      s.oi = 0;
      if (!reserve_objects(s, max_n)) return;
      s.ph = PH_PREPALL;                                     // (the grouping by object rode in the cluster launch)
      return;
    }
    if (s.ph == PH_PREPALL_WAIT) {
      const uint32_t* nv = ws->m_nvalid.as<uint32_t>();
      for (size_t i = 0; i < s.objs.size(); ++i) {
        s.objs[i].nvalid = nv[4 * i]; s.objs[i].degsum = nv[4 * i + 1]; s.objs[i].triangle = nv[4 * i + 2];
      }
      s.ph = PH_OBJECT;
      return;
    }
    if (s.ph == PH_PREP_WAIT) {                             // a further round of the same object, after an accepted pose
      start_round(s, m->prep[0], m->prep[1], m->prep[2]);
      return;
    }
    if (s.ph == PH_DRAW_WAIT) {
      if (eval_failed(s)) return;                           // (the evaluation of this walk's iterations ran in the same tick)
      const ChainOut co = m->chain;
      TOD_DBG2("  draw window: S=%u len=%u -> done=%u pos_end=%u attempts=%u flag=%u", r.S, r.window_len, co.n_done, co.pos_end,
              co.attempts, co.flag);
      uint32_t* hp = ws->m_pos.as<uint32_t>();             // positions of this walk are relative to the window start
      for (uint32_t i = 0; i < co.n_done; ++i) hp[r.it_begin + r.got + i] += (uint32_t)r.consumed;
      r.got += co.n_done;
      r.consumed += co.pos_end;
      r.attempts_carry = co.attempts;
      if (co.flag == 2) {
        r.selection_empty = true;
        // the walk that just gave up consumed r.consumed draws in all: the next object's first window covers that much
        uint32_t hint = 1024u;
        while (hint < r.consumed + 512u && hint < (1u << 20)) hint <<= 1;
        s.s_hint = std::max(s.s_hint, hint);
      }
      if (co.flag == 1) r.s_floor = std::min<uint32_t>(std::max(r.S, 1024u) * 4u, 1u << 20);   // e.g. 1000 failing attempts in a row
      if (co.flag == 1 && co.n_done == 0 && co.pos_end == 0) {
        // a single attempt longer than the window: enlarge the look-ahead, give up beyond 64M draws
        if (r.lookahead >= (1u << 26)) { fail(s, TODHIP_ESCRATCH); return; }
        r.lookahead *= 4u;
      }
      if (r.got < r.want && !r.selection_empty) s.ph = PH_DRAW; else after_draw(s);
      return;
    }
    if (s.ph == PH_EVAL2_WAIT) {
      if (eval_failed(s)) return;
      eval_done(s, true);
      return;
    }
    if (s.ph == PH_SPRINT_WAIT) { consume_sprint(s); return; }
    if (s.ph == PH_GROWTH_WAIT) {
      const GrowthOut* go = &m->growth;
      TOD_DBG2("  growth: model=%u matches=%u kps=%u passes=%u", go->n_model_inliers, go->n_match_inliers, go->n_kp_inliers,
              go->passes);
      round_done(s, true);
      return;
    }
  }

  bool reserve_objects(Slot& s, uint32_t max_n) {
    VerifyWs* ws = s.ws;
    if (max_n > (uint32_t)kMaxWords * 64u) { fail(s, TODHIP_ESCRATCH); return false; }
    uint64_t adj = 0, bits = 0, deg = 0;
    for (ObjSpan& o : s.objs) {
      if (o.n < 3) continue;
      const uint64_t W = (o.n + 63u) / 64u;
      o.adj_off = adj; o.bits_off = (uint32_t)bits; o.deg_off = (uint32_t)deg;
      adj += (uint64_t)o.n * W; bits += 8u * W; deg += o.n;
    }
    const size_t n_objs_here = std::max<size_t>(s.objs.size(), 1);
    if (ws->phys.reserve((size_t)std::max<uint64_t>(adj, 1) * 8) != hipSuccess || ws->samp.reserve((size_t)std::max<uint64_t>(adj, 1) * 8) != hipSuccess ||
        ws->bits.reserve((size_t)std::max<uint64_t>(bits, 8) * 8) != hipSuccess || ws->sampdeg.reserve((size_t)std::max<uint64_t>(deg, 1) * 4) != hipSuccess ||
        ws->nvalid.reserve(n_objs_here * 16) != hipSuccess || ws->m_nvalid.reserve(n_objs_here * 16) != hipSuccess) {
      fail(s, TODHIP_EHIP);
      return false;
    }
    return true;
  }

  int reserve_common(Slot& s) {
    VerifyWs* ws = s.ws;
    const uint32_t kp_words = (nq + 63u) / 64u;
    TOD_HIP(ws->small.reserve(256 * sizeof(uint32_t)));
    TOD_HIP(ws->m_small.reserve(kMailSmallWords * sizeof(uint32_t)));
    TOD_HIP(ws->kp_bits.reserve((size_t)(kp_words + 1) * sizeof(u64)));
    TOD_HIP(ws->m_kp.reserve((size_t)std::max(nq, 1u) * sizeof(uint32_t)));
    VerifyPool* pool = tod_ws<VerifyPool>(ctx);
    if (!pool->kceil_ready) {
      // ransac_k per (|valid|, n_best), once: `iterations_ < k` (ransac.h:95) is `iterations_ < ceil(k)` for an integer
      // iterations_, so the device replays the loop test exactly from this table
      std::vector<uint32_t> tab(65u * 65u, 1u);
      for (uint32_t nv = 1; nv <= 64u; ++nv)
        for (uint32_t nb = 0; nb <= 64u; ++nb) {
          const double c = std::ceil(ransac_k((double)(int)nb / (double)nv));
          tab[nv * 65u + nb] = c >= 2147483647.0 ? 0x7FFFFFFFu : (uint32_t)c;
        }
      TOD_HIP(pool->kceil.reserve(tab.size() * sizeof(uint32_t)));
      TOD_HIP(hipMemcpy(pool->kceil.p, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
      pool->kceil_ready = true;
    }
    return TODHIP_OK;
  }
  int reserve_cluster(Slot& s) {
    VerifyWs* ws = s.ws;
    const size_t cap = (size_t)nq * k;
    TOD_HIP(ws->c_kept.reserve((size_t)nq * 4)); TOD_HIP(ws->c_offs.reserve(((size_t)nq + 1) * 4));
    TOD_HIP(ws->c_qpt.reserve((size_t)nq * 12)); TOD_HIP(ws->c_obj.reserve(cap * 4));
    TOD_HIP(ws->c_hist.reserve((size_t)n_objs * 4)); TOD_HIP(ws->c_goff.reserve((size_t)n_objs * 4));
    TOD_HIP(ws->c_src.reserve(cap * 4)); TOD_HIP(ws->c_cnt.reserve((size_t)n_objs * 4));
    TOD_HIP(ws->m_hist.reserve((size_t)n_objs * 4));
    TOD_HIP(ws->train.reserve(cap * 12)); TOD_HIP(ws->query.reserve(cap * 12));
    TOD_HIP(ws->qidx.reserve(cap * 4)); TOD_HIP(ws->kpxy.reserve(cap * 8));
    return TODHIP_OK;
  }

  // first-pass LDS per hypothesis: the induced graph has at most n vertices, so a small object does not need the
  // whole 48 KB carve (adjacency + colouring scratch + 4 KB of level stack) and more hypotheses fit a CU at once
  static uint32_t eval_lds_small(uint32_t n) {
    const uint32_t W = (n + 63u) / 64u;
    const uint32_t want = gate_lds_bytes(n) + 8u * n * W + 4096u;
    return std::min(kEvalLdsSmall, std::max(8192u, (want + 1023u) & ~1023u));
  }

  // ==== the launcher: a tick's argument lists -> launches
  // A list of thousands of argument sets (the all-objects preparation tick of a batch: ~190 objects per frame): the sets go to
  // device memory in one copy, ordered by size class so that a launch's grid -- the extent of its largest member times the
  // count -- stays tight, and each class is ONE launch (252 launches of <= 36 sets each became 3-4 per kernel). `used` = bytes
  // of the staging area already taken in this tick.
  template <class A, class KernP, class Extent>
  bool launch_many(hipStream_t st, KernP kern, const std::vector<A>& v, int slot_dim, Extent extent, size_t& used, uint32_t block, uint32_t lds,
                   bool by_class) {
    VerifyPool* pool = tod_ws<VerifyPool>(ctx);
    HostBuf& args_stage = pool->args_stage[lane_now];
    DevBuf& args_dev = pool->args_dev[lane_now];
    const size_t bytes = v.size() * sizeof(A);
    used = (used + 255u) & ~(size_t)255u;
    if (used + bytes > args_stage.cap || used + bytes > args_dev.cap) return false;
    static const uint32_t kClassBy[] = {16u, 64u, 256u, 0xFFFFFFFFu}, kClassOne[] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    const uint32_t* kClass = by_class ? kClassBy : kClassOne;
    A* host = reinterpret_cast<A*>(reinterpret_cast<unsigned char*>(args_stage.p) + used);
    const A* dev = reinterpret_cast<const A*>(reinterpret_cast<const unsigned char*>(args_dev.p) + used);
    size_t n_cls[4] = {0, 0, 0, 0}, at = 0;
    auto cls_of = [&](const A& a) { uint32_t c = 0; while (a.job.n > kClass[c]) ++c; return c; };
    for (const A& a : v) ++n_cls[cls_of(a)];
    size_t start[4], fill[4];
    for (int c = 0; c < 4; ++c) { start[c] = fill[c] = at; at += n_cls[c]; }
    for (const A& a : v) host[fill[cls_of(a)]++] = a;
    if (hipMemcpyAsync(const_cast<A*>(dev), host, bytes, hipMemcpyHostToDevice, st) != hipSuccess) return false;
    used += bytes;
    for (int c = 0; c < 4; ++c) {
      for (size_t i0 = 0; i0 < n_cls[c]; i0 += 32768u) {    // (grid z / y limit)
        const uint32_t n = (uint32_t)std::min<size_t>(32768u, n_cls[c] - i0);
        uint32_t gx = 1, gy = 1;
        for (uint32_t i = 0; i < n; ++i) { const dim3 e = extent(host[start[c] + i0 + i]); gx = std::max(gx, e.x); gy = std::max(gy, e.y); }
        const dim3 grid = slot_dim == 1 ? dim3(gx, n) : dim3(gx, gy, n);
        SlotsPtr<A> S = {dev + start[c] + i0};
        hipLaunchKernelGGL(kern, grid, dim3(block), lds, st, S);
      }
    }
    return true;
  }

  // One list, launched in one of the two forms of passing argument sets: staged in device memory (launch_many with kern_ptr) when
  // the caller says the list is long and the tick's staging reserve succeeded, by value in kernarg (launch_list<N> with kern_val)
  // otherwise -- also when launch_many declines.
  struct Staging { bool ok = false; size_t used = 0; };     // the lane's staging area in this tick: reserved? bytes taken
  template <uint32_t N, class A, class KernP, class KernV, class Extent>
  void launch_either(hipStream_t st, KernP kern_ptr, KernV kern_val, const std::vector<A>& v, bool long_list, Staging& stage, int slot_dim,
                     Extent extent, uint32_t block, uint32_t lds, bool by_class) {
    if (long_list && stage.ok && launch_many(st, kern_ptr, v, slot_dim, extent, stage.used, block, lds, by_class)) return;
    launch_list<N>(st, kern_val, v, block, lds, slot_dim, extent);
  }
#define TOD_BOTH_FORMS(kern, A, N) kern<SlotsPtr<A>>, kern<Slots<A, N>>

  template <class F>
  static void split_evals(const std::vector<EvalArgs>& v, uint32_t lds, bool deferred, F& launch_evals) {
    bool any_wide = false, any_narrow = false;
    for (const EvalArgs& a : v) (a.job.W <= 8u ? any_narrow : any_wide) = true;
    if (any_wide && any_narrow) { launch_evals(v, true, lds, deferred); return; }
    launch_evals(v, any_wide, lds, deferred);
  }
  void launch_all(hipStream_t st) {
    // the staging area for argument sets in device memory (launch_many) is sized once per tick, before anything reads it
    Staging stage;
    {
      const size_t n_eval = L.eval_small.size() + L.eval_direct.size() + L.eval_big.size();
      if (L.adj.size() > 4u * kManySlots || n_eval > kMaxSlots || L.prep_small.size() > kManySlots) {
        VerifyPool* pool = tod_ws<VerifyPool>(ctx);
        const size_t need = L.finite.size() * sizeof(JobArgs) + L.adj.size() * sizeof(AdjArgs) + L.prep.size() * sizeof(PrepArgs) +
                            L.prep_small.size() * sizeof(PrepSmallArgs) + n_eval * sizeof(EvalArgs) + 4096u;
        stage.ok = pool->args_stage[lane_now].reserve(need) == hipSuccess && pool->args_dev[lane_now].reserve(need) == hipSuccess;   // (the lane is idle)
      }
    }
    // more hypothesis evaluations than fit one launch's arguments (a batch of more than 16 frames): one launch all the same
    auto launch_evals = [&](const std::vector<EvalArgs>& v, bool wide, uint32_t lds, bool deferred) {
      pick_eval(wide, deferred, [&](auto kern_ptr, auto kern_val, auto ext) {
        launch_either<kMaxSlots>(st, kern_ptr, kern_val, v, v.size() > kMaxSlots, stage, 1, ext, 64u, lds, false);
      });
    };
    auto words = [](const CopyArgs& a) { return dim3(std::max(1u, std::min(64u, (a.n + 255u) / 256u))); };
    L.copy_in.insert(L.copy_in.end(), L.zero.begin(), L.zero.end());   // both precede every other kernel of the tick: one launch
    launch_list<kCopySlots>(st, copy_words_kernel, L.copy_in, 256, 0, 1, words);
    for (size_t i = 0; i < L.sprint.size(); ++i) { L.sprint[i].rnd = L.sprint_src[i]->dev.as<uint32_t>(); L.sprint[i].rnd_len = L.sprint_src[i]->dev_valid; }
    launch_list<kWideSlots>(st, sprint_kernel, L.sprint, kSprintThreads, kSprintLds, 0, [](const SprintArgs&) { return dim3(1); });
    launch_list(st, cluster_frame_kernel, L.cluster, 256, 0, 0, [](const ClusterArgs&) { return dim3(1); });
    launch_list(st, cluster_frame_rescaled_kernel, L.cluster_rescaled, 256, 0, 0, [](const ClusterRescaledArgs&) { return dim3(1); });
    launch_list<kWideSlots>(st, invalidate_kernel, L.inval, 256, 0, 0, [](const InvArgs&) { return dim3(1); });
    launch_either<kManySlots>(st, TOD_BOTH_FORMS(small_prep_kernel, PrepSmallArgs, kManySlots), L.prep_small, L.prep_small.size() > kManySlots, stage,
                              1, [](const PrepSmallArgs&) { return dim3(1); }, 64u, 0u, false);
    {
      auto ext_rows = [](const auto& a) { return dim3((a.job.n + 255u) / 256u); };
      auto ext_adj = [](const AdjArgs& a) { return dim3(a.job.n, (a.job.W + 3u) / 4u); };
      const bool many = L.adj.size() > 4u * kManySlots;    // the all-objects preparation of a batch: its three lists go together
      launch_either<kManySlots>(st, TOD_BOTH_FORMS(finite_kernel, JobArgs, kManySlots), L.finite, many, stage, 1, ext_rows, 256u, 0u, true);
      launch_either<kManySlots>(st, TOD_BOTH_FORMS(adjacency_kernel, AdjArgs, kManySlots), L.adj, many, stage, 2, ext_adj, 256u, 0u, true);
      launch_either<kManySlots>(st, TOD_BOTH_FORMS(round_prep_kernel, PrepArgs, kManySlots), L.prep, many, stage, 1, ext_rows, 256u, 0u, true);
    }
    for (int f = DRAW_FORMS - 1; f >= 0; --f) {              // (the wave forms first, as before)
      for (size_t i = 0; i < L.draw[f].size(); ++i) L.draw[f][i].rnd = L.draw_src[f][i].first->dev.as<uint32_t>() + L.draw_src[f][i].second;
      launch_draws(st, (DrawForm)f, L.draw[f]);
    }
    {
      // dynamic LDS: the packed hop words of the largest window of the launch + the per-iteration start positions
      uint32_t lds = 0;
      for (const ChainArgs& c : L.chain) lds = std::max(lds, (std::min(c.S, kChainLdsEntries) + std::min(c.n_req, kChainMaxReq)) * 4u);
      launch_list<kWideSlots>(st, chain_kernel, L.chain, 256, lds, 0, [](const ChainArgs&) { return dim3(1); });
    }
    {
      // one dynamic LDS size per launch: the largest any slot of the launch wants; every slot carves that much
      uint32_t lds = 8192u;
      for (const EvalArgs& a : L.eval_small) lds = std::max(lds, a.lds_bytes);
      for (EvalArgs& a : L.eval_small) a.lds_bytes = lds;
      // objects of more than 512 matches need the kernel's wide instantiation. It serves the smaller ones as well (6 % slower than
      // their own instantiation): when a tick holds both kinds -- the frames of a batch reach objects of 340 and of 590 matches
      // together -- one launch for all of them instead of two in a row, each as long as its slowest clique search
      split_evals(L.eval_small, lds, false, launch_evals);
    }
    split_evals(L.eval_direct, kEvalLdsBig, false, launch_evals);
    split_evals(L.eval_big, kEvalLdsBig, true, launch_evals);
    launch_list(st, growth_kernel, L.growth, 256, 0, 0, [](const GrowthArgs&) { return dim3(1); });
    launch_list<kWideSlots>(st, invalidate_kernel, L.inval_after, 256, 0, 0, [](const InvArgs&) { return dim3(1); });
    launch_list<kManySlots>(st, round_prep_kernel<Slots<PrepArgs, kManySlots>>, L.prep_after, 256, 0, 1, [](const PrepArgs& a) { return dim3((a.job.n + 255u) / 256u); });
    launch_list<kCopySlots>(st, copy_words_kernel, L.copy_out, 256, 0, 1, words);
    L = Launches();
  }
#undef TOD_BOTH_FORMS

  // ==== the lane scheduler: which slots launch together, on which stream, and when they consume
  // slots: live frames (phase set by the caller). Returns the first slot error, if any.
  int run(std::vector<Slot*>& slots) {
    // stream caches live in the context (a harness that restarts rand() per frame reuses one stream for ever); a
    // few of the most recent start states are kept
    std::vector<StreamCache*>& caches = tod_ws<VerifyPool>(ctx)->streams;
    for (Slot* s : slots) {
      s->start_draws = s->rng->draws; s->abs_pos = 0; s->stream = nullptr;
      for (StreamCache* c : caches) if (c->same_start(*s->rng)) { s->stream = c; break; }
      if (!s->stream) {
        if (caches.size() >= 64) {                          // none of the live slots can be using the oldest ones
          bool in_use = false;
          for (Slot* t : slots) in_use = in_use || t->stream == caches.front();
          if (!in_use) { TOD_HIP(hipStreamSynchronize(st)); caches.front()->dev.release(); delete caches.front(); caches.erase(caches.begin()); }
        }
        caches.push_back(new StreamCache(*s->rng));
        s->stream = caches.back();
      }
    }
    const int rc_run = run_ticks(slots);
    for (Slot* s : slots) {                                 // the caller's generator ends where the reference's would
      if (s->abs_pos) { const uint64_t d0 = s->start_draws; *s->rng = s->stream->state_at(s->abs_pos); s->rng->draws = d0 + s->abs_pos; }
      s->stream = nullptr;
    }
    return rc_run;
  }
  // A launch group = the slots that are ready at one moment and in the same kind of phase: each issues the kernels of its next
  // phase, the lists are launched once for all of them on an idle LANE (the context's stream, or one of the process's few side
  // streams), an event is recorded, and when it has fired every slot of the group consumes its results. The host never blocks on one
  // group while another could be consumed or launched: the frames of a batch reach their sprints, their big object's clique gates
  // (a single wave for most of a millisecond) and its growth at different moments, and a kernel of one kind queued behind a long one
  // of another kind on the same stream would wait for it. With one lane (a lone frame, or more than two batches in the air in this
  // process: their contexts' streams already overlap each other) this is the plain lock-step tick: everything ready in one launch,
  // one wait. Nothing here changes what a slot computes or in which order it consumes it.
  static constexpr uint32_t kHeavyN = 96;                  // matches of an object from which its evaluation / growth is a kind of its own
  enum Kind { K_LIGHT = 0, K_GROWTH = 1, K_SPRINT = 2, K_EVAL = 3, K_COUNT = 4 };
  static Kind kind_of(const Slot& s) {
    if (s.ph == PH_OBJECT) {                                // its next launch: a sprint, or the first evaluation of a big object
      size_t i = s.oi;                                      // (the objects PH_OBJECT decides without a kernel are skipped)
      while (i < s.objs.size() && !s.objs[i].resume && (s.objs[i].n < 3u || s.objs[i].nvalid < 3u || !s.objs[i].triangle)) ++i;
      if (i >= s.objs.size()) return K_LIGHT;
      if (sprint_on() && sprint_live(s.objs[i])) return K_SPRINT;
      return s.objs[i].n >= kHeavyN ? K_EVAL : K_LIGHT;
    }
    if ((s.ph == PH_DRAW || s.ph == PH_EVAL2) && s.job.n >= kHeavyN) return K_EVAL;
    if (s.ph == PH_GROWTH && s.job.n >= kHeavyN) return K_GROWTH;
    return K_LIGHT;
  }
  static uint32_t n_side_streams() {
    static const uint32_t n = [] {
      const char* e = getenv("TODHIP_VERIFY_FLIGHTS");
      const long v = e ? strtol(e, nullptr, 10) : 2;
      return (uint32_t)std::min<long>(std::max<long>(v, 0), 16);
    }();
    return n;
  }
  void describe(char* what, size_t cap) const {
    snprintf(what, cap, "lookup %zu adj %zu prep %zu draw %zu+%zu chain %zu eval %zu+%zu growth %zu inval %zu sprint %zu", L.cluster.size() + L.cluster_rescaled.size(),
             L.adj.size() + L.prep_small.size(), L.prep.size() + L.prep_small.size(), L.draw[DRAW_WAVE1].size() + L.draw[DRAW_WAVE8].size(), L.draw[DRAW_LANE2].size() + L.draw[DRAW_LANE8].size(), L.chain.size(), L.eval_small.size() + L.eval_direct.size(),
             L.eval_big.size(), L.growth.size(), L.inval.size(), L.sprint.size());
  }
  struct Lane {
    hipStream_t st; hipEvent_t ev; std::atomic<bool>* taken;   // taken: a side stream of the process, claimed while a group is on it
    std::vector<Slot*> slots; bool busy = false; std::chrono::steady_clock::time_point t0; char what[128];
  };
  int run_ticks(std::vector<Slot*>& slots) {
    struct InAir { InAir() { n = g_batches_in_air.fetch_add(1) + 1; } ~InAir() { g_batches_in_air.fetch_sub(1); } int n; } in_air;
    VerifyPool* pool = tod_ws<VerifyPool>(ctx);
    std::vector<hipStream_t> side;
    SideStreams::PerDevice* pd = nullptr;
    if (slots.size() > 1 && in_air.n <= 2 && n_side_streams() > 0) TOD_HIP(g_side_streams.get(ctx->device, n_side_streams(), side, &pd));
    while (pool->side_ev.size() < side.size() + 1) {
      hipEvent_t e2;
      TOD_HIP(hipEventCreateWithFlags(&e2, hipEventDisableTiming));
      pool->side_ev.push_back(e2);
    }
    std::vector<Lane> lanes(1 + side.size());
    lanes[0].st = st; lanes[0].ev = pool->side_ev[0]; lanes[0].taken = nullptr;
    for (size_t i = 0; i < side.size(); ++i) { lanes[1 + i].st = side[i]; lanes[1 + i].ev = pool->side_ev[1 + i]; lanes[1 + i].taken = &pd->taken[i]; }
    auto drain = [&]() {
      for (Lane& ln : lanes) if (ln.busy) { (void)hipEventSynchronize(ln.ev); ln.busy = false; if (ln.taken) ln.taken->store(false); }
    };
#define LOOP_HIP(expr) do { if ((expr) != hipSuccess) { drain(); return TODHIP_EHIP; } } while (0)
    std::vector<Slot*> ready[K_COUNT];
    while (true) {
      // groups that have landed: their slots consume and are ready again
      bool any_busy = false;
      for (Lane& ln : lanes) {
        if (!ln.busy) continue;
        const hipError_t q = hipEventQuery(ln.ev);
        if (q == hipErrorNotReady) { any_busy = true; continue; }
        LOOP_HIP(q);
        ln.busy = false;
        if (ln.taken) ln.taken->store(false);
        if (tod_debug())
          TOD_DBG("tick %.1f us: %s (lane %zu, %zu slots)", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - ln.t0).count(),
                  ln.what, (size_t)(&ln - lanes.data()), ln.slots.size());
        for (Slot* s : ln.slots) { s->in_flight = false; if (s->ph != PH_DONE) consume(*s); }
        ln.slots.clear();
        TOD_DBG("consumed");
      }
      for (auto& r : ready) r.clear();
      size_t n_ready = 0;
      for (Slot* s : slots) {
        if (s->ph == PH_DONE || s->in_flight) continue;
        ready[lanes.size() > 1 ? kind_of(*s) : K_LIGHT].push_back(s);
        ++n_ready;
      }
      if (n_ready == 0 && !any_busy) break;
      // every kind of ready slots takes an idle lane of its own; a kind that finds none waits for the next landing
      bool launched = false;
      for (int k = 0; k < K_COUNT && n_ready; ++k) {
        if (ready[k].empty()) continue;
        Lane* ln = nullptr;
        for (Lane& c : lanes) {
          if (c.busy) continue;
          if (c.taken) { bool expected = false; if (!c.taken->compare_exchange_strong(expected, true)) continue; }   // another context has it
          ln = &c;
          break;
        }
        if (!ln) break;
        lane_now = (size_t)(ln - lanes.data());
        for (Slot* s : ready[k]) {
          issue(*s);
          if (s->ph != PH_DONE) { s->in_flight = true; ln->slots.push_back(s); }
        }
        if (ln->slots.empty()) { L = Launches(); if (ln->taken) ln->taken->store(false); launched = true; continue; }   // (they finished without a kernel)
        if (tod_debug()) { describe(ln->what, sizeof(ln->what)); ln->t0 = std::chrono::steady_clock::now(); }
        launch_all(ln->st);
        const hipError_t e1 = hipGetLastError();
        const hipError_t e2 = e1 == hipSuccess ? hipEventRecord(ln->ev, ln->st) : e1;
        if (e2 != hipSuccess) { if (ln->taken) ln->taken->store(false); for (Slot* s : ln->slots) s->in_flight = false; ln->slots.clear(); drain(); return TODHIP_EHIP; }
        ln->busy = true;
        launched = true;
        ctx->counters.last_verify_ticks += 1;
      }
      if (launched) continue;                                // (slots that finished without a kernel may be ready for more)
      // nothing could be launched: wait for the first group to land
      bool landed = false;
      while (!landed) {
        bool busy_now = false;
        for (Lane& ln : lanes) {
          if (!ln.busy) continue;
          busy_now = true;
          const hipError_t q = hipEventQuery(ln.ev);
          if (q == hipSuccess) { landed = true; break; }
          if (q != hipErrorNotReady) LOOP_HIP(q);
        }
        if (!busy_now) break;                                // every lane is idle (another context holds the side streams): try again
        if (!landed) std::this_thread::yield();
      }
    }
#undef LOOP_HIP
    for (Slot* s : slots)
      if (s->rc != TODHIP_OK) return s->rc;
    return TODHIP_OK;
  }
#undef SLOT_HIP
};
