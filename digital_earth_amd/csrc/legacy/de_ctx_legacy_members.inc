// members of struct de_ctx that only the legacy kernel families use (included inside the struct by de_context.h under DE_LEGACY_VARIANTS):
// the wavefront pipeline's pipes and launch policy (rounds 3-4), the HBM-queue scheduler's launch state and knobs (round 4).
    // render_kernel_v3: one "pipe" = a set of stage queues + cold records.  Two pipes let two batches of paths run side by side on
    // two launch slots, so that the tail-heavy small launches of one overlap the large launches of the other (env DE_V3_PIPES)
    struct V3Pipe {
        Dev<wf::Rec> rec[wf::NQ];   // stage queues (64 B per path each)
        Dev<uint32_t> ctl;           // two sets of 2 control words per queue (the set being filled / the set to fill next)
        int epoch[wf::NQ] = {0, 0, 0, 0, 0, 0, 0};   // completed drains per queue: parity selects the current set
        Dev<wf::Cold> cold;          // 64 B per path
        size_t capacity = 0;          // paths the buffers hold
        // statistic for the automatic variant: records queued for vertex round 2 (holes included) of one launch, copied to pinned
        // host memory in stream order and read by a LATER de_accumulate call — never waited for
        Pinned<uint32_t> h_round2;
        hipEvent_t stat_ev = nullptr, ev_t[3] = {nullptr, nullptr, nullptr};   // stat_ev: the copy has landed; ev_t: start / pipeline done / finisher done
        bool stat_pending = false, stat_timed = false;
        unsigned long long stat_items = 0;
        int stat_pipes = 1;
    } v3p[4];
    float auto_ratio = -1.f;         // last known (records queued for round 2) / (paths started); < 0 = none yet
    // Calls between auto_min_items and the two-pipe size (a rank's share of a tile partition, accumulate(16)) run the pipeline on four
    // pipes.  Rounds 3 picked the kernel for them by timing 32 calls on each (the state machine alone was 2-10 % faster on light views);
    // since the cloud stage reuses its map footprints (round 4) the pipeline wins or ties on every camera and share measured
    // (profiles/experiments: world 2 / 4 / 8 x four cameras; worst case -4 % / -9 % on the default / Apollo camera at 1/8 frame against
    // +24 % ... +45 % elsewhere), so the measuring state machine is gone.  env DE_AUTO_MID: 1 = the pipeline (default), 2 = the state machine
    int auto_mid_mode = 1;
    float auto_ns_per_path = -1.f;   // last known duration of a pipeline launch / its paths / the pipes running side by side
    bool auto_deep = false;          // the deep setting is in use (hysteresis: entered above auto_deep_ns, left below 0.8 x)
    int v3_pipes = 1;
    int v3_finisher = 2;             // what finishes the paths the pipeline hands over: 2 = render_kernel_v2 (resume mode), 5 = render_kernel_v5 (env DE_V3_FINISHER)
    int v5_fin_wpc = 8;              // waves per CU of a finisher launch of render_kernel_v5 (two pipes side by side; env DE_V5_FIN_WPC)
    int v3_fuse_track = 0;           // 1: one kernel tracks a ray through the gases and on through the cloud shell (v3_track_kernel: bit-identical, measured 8 % slower: profiles/experiments); 0: two stage kernels (env DE_V3_FUSE_TRACK)
    int v3_depths = 25;              // vertex rounds run by the pipeline before render_kernel_v2 finishes the surviving paths (env DE_V3_DEPTHS; 25 = all)
    int v3_batches = 2;              // with two pipes: batches a call is cut into (they alternate between the pipes; env DE_V3_BATCHES)
    size_t v3_max_items = (size_t)1 << 27;   // paths per batch (512 B each: 68 GB per pipe at 2^27 = a whole 1920x1080x64-spp frame; v3_reserve asks the device first and the batch shrinks when there is no room); env DE_V3_MAX_ITEMS
    size_t v3_test_budget = 0;       // env DE_V3_TEST_BUDGET (paths): see v3_reserve
    int v3_slack_wpc = 14;           // the largest wave budget any stage grid may get (set after the env knobs are read): sizes the queues' room for holes
    int v3_wpc = 14;                 // waves per CU the v3 grids are sized for (env DE_V3_WPC; per class: DE_V3_WPC_ST / _GAS / _CLOUD / _FLAT).
                                     // NOT the 32 the CU can hold: 64 paths per wave each keep a map line hot between two steps, and
                                     // beyond ~14 waves per CU that working set outgrows the XCD's 4 MB L2 (334 ms at 32, 252 ms at 14)
    int v3_wpc_class[4] = {0, 0, 16, 0};  // 0 = the call's wave budget; index: 0 sphere trace (and primary), 1 gas, 2 cloud, 3 the straight-line stages.  Cloud: 16 since the
                                          // tracking steps reuse their map footprint (round 4): the stage no longer lives on L2 capacity (8 / 12 / 16 / 20 / 24 / 32 waves: 186 / 176 / 174.5 / 181 / 180 / 186 ms per step)
    // render_kernel_v5 (kernel variant 5): one persistent stage-scheduler launch per call.  Each launch slot that runs it owns a chunk
    // pool, the queue rings, the control words and the cold records of its launch (launches of different slots overlap).
    struct V5State {
        Dev<uint4> pool;
        Dev<uint32_t> ctl, rings, free_ring;
        Dev<unsigned long long> cold;
        Dev<RenderArgs> d_args;           // the launch's RenderArgs (written by v5_init_kernel)
        Pinned<uint32_t> h_status;        // pinned, device-visible: the kernel's abort code
        size_t cold_items = 0;
        uint32_t pool_chunks = 0, ring_cells = 0, n_shards = 0;
    } v5s[DE_MAX_SLOTS + 4];         // one per launch slot (kernel variant 5), then one per pipe (the pipeline's finisher, v3_finisher = 5)
    int v5_wpc = 16;                 // waves per CU of the persistent grid (env DE_V5_WPC)
    int v5_shards = 32;              // queue sets (8 = one per XCD; env DE_V5_SHARDS)
    int v5_local = 1;                // 1: teams live inside an XCD when the shard count is a multiple of 8 (env DE_V5_LOCAL)
    int v5_backlog = 2;              // chunks per wave queued in a shard before the waves stop starting new paths (env DE_V5_BACKLOG)
    int v5_pool_log2 = 18;           // chunks of 64 records in a slot's pool (2^18 = 1 GB; env DE_V5_POOL_LOG2)
    int v5_claim_k = 16, v5_age = 20000, v5_closers_per_cu = 2, v5_stats = 0;   // env DE_V5_CLAIM_K / _AGE (10 ns ticks) / _CLOSERS / _STATS
    int v5_reserve_pct = 25;         // new paths start only while this share of the pool is free (env DE_V5_RESERVE_PCT)
    size_t v5_max_items = (size_t)1 << 27;   // paths per launch (64 B of cold record each; env DE_V5_MAX_ITEMS)
    int v5_batches = 1;              // launches a large call is cut into (they overlap on the launch slots; env DE_V5_BATCHES)
    // variant 4 (automatic).  Measured on BASELINE's cameras (1920x1080, profiles/r3d_summary.md, profiles/experiments/): three vertex
    // rounds in the pipeline + the state machine as finisher beat the state machine alone by 7 % (default camera, 64 spp) to 77 %
    // (limb view), with 8 waves per CU per pipe, two pipes for batches above 48 M paths and four below (small batches: more tails to
    // overlap; large ones: the L2 holds two batches' lines, not four); launches under 8 M paths (the interactive 1-spp call) stay
    // with the state machine and its launch slots.
    int auto_depths = 3, auto_wpc = 8, auto_pipes = 0;
    int auto_full_batches1 = 1;      // 1: a full-frame call issued while others are in flight, outside the deep setting, is one batch (env DE_AUTO_FULL_BATCHES1)
    int auto_mid_batches1 = 1;       // 1: a mid-size call issued while others are in flight is one batch on one pipe (env DE_AUTO_MID_BATCHES1)
    unsigned long long auto_lone_max_items = 1ull << 23;    // largest lone call that runs the persistent scheduler (env DE_AUTO_LONE_MAX_ITEMS): the small calls.
                                                            // Up to 40 M paths it would still win on latency (a lone 1/8 share 34.2 against 43.7 ms, 1/4 share 56.0 / 65.1), but the
                                                            // first call of every back-to-back run is a lone one, and a persistent launch ahead of pipeline launches cost such runs
                                                            // 3-8 % (12 steps of the 1/4 share: 46.2 against 42.8 ms per step): not by default
    int auto_budget_v5 = 1;          // 1: a call the memory budget keeps off the pipeline runs the persistent scheduler when that fits (env DE_AUTO_BUDGET_V5)
    int auto_lone_v5 = 1;            // 1: a small call that finds nothing of this context in flight runs the persistent scheduler (env DE_AUTO_LONE_V5)
    unsigned long long auto_min_items = 1ull << 23, auto_two_pipe_items = 48ull << 20;
    // views whose paths are long (limb views through thick cloud: 2.4 - 2.9 ns of GPU time per path against 1.0 - 1.4 for the default camera)
    // keep the stage kernels full for more rounds and amortise a third, smaller batch: the pipeline then runs auto_deep_depths
    // rounds on auto_deep_pipes pipes (env DE_AUTO_DEEP_NS in 1/100 ns per path / DE_AUTO_DEEP_DEPTHS / DE_AUTO_DEEP_PIPES)
    int auto_deep_ns_x100 = 200, auto_deep_depths = 5, auto_deep_pipes = 3;
    int last_v3_slot[4] = {-1, -1, -1, -1};  // a pipe's launches follow each other
