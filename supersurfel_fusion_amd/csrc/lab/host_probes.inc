// lab/host_probes.inc -- PROBE ENTRY POINTS of the host code (ablation timers, fault injection, record dumps for tools/), compiled
// only with -DSSF_EXPERIMENTS (csrc/variants/lab; `make lab`): none is part of the product library.  Included by ssf_host.hip at the
// end of its extern "C" block, so they reach that file's statics (submit_extract, activate_oldest, retire_active, now_us).

// the record of the last ICP iteration the host fetched (after the exchange of a sharded map: the SUM over the ranks)
int ssf_dbg_last_icp_record(ssf_handle* h, int64_t* out29) {
    if (!h || !out29) return SSF_ERR_INVALID_ARG;
    for (int i = 0; i < 29; i++) out29[i] = h->h_icp_local[i];
    return SSF_OK;
}
// device copy of the last record [0..28] and, with the peer-to-peer exchange, of this shard's own record before it [32..60]
int ssf_dbg_device_icp_records(ssf_handle* h, int64_t* out64) {
    if (!h || !out64) return SSF_ERR_INVALID_ARG;
    HCK(hipStreamSynchronize(h->stream));
    HCK(hipMemcpy(out64, h->d_icp, 64 * sizeof(int64_t), hipMemcpyDeviceToHost));
    return SSF_OK;
}
// fault injection: a stall of the calling thread in front of the host's word to the waiting launch (ssf_waiter_match_repairs)
void ssf_dbg_stall_before_match_us(ssf_handle* h, long long us) { if (h) h->dbg_stall_before_match_us = us; }
// frames whose in-launch association bid into the replicas of the association table (SSF_ASSOC_REPLICAS=0 switches them off)
long long ssf_dbg_assoc_replica_frames(ssf_handle* h) { return h ? h->n_assoc_replica_frames : -1; }
// host-side time split of the pipelined loop (tools/pipeline_probe.py); reset on read
int ssf_dbg_host_times(ssf_handle* h, double* out8) {
    if (!h || !out8) return SSF_ERR_INVALID_ARG;
    for (int i = 0; i < 8; i++) { out8[i] = h->host_us[i]; h->host_us[i] = 0; }
    return SSF_OK;
}
// throughput of the extract stage alone (tools/extract_only_probe.py): frames (device pointers, `nlist` of them,
// cycled) go through the batch contexts and are retired unread; returns microseconds per frame.  The handle's
// frame stamp advances as if the frames had been fused.
double ssf_dbg_extract_only(ssf_handle* h, const void* const* rgb, const void* const* depth, int nlist, int n) {
    if (!h || !rgb || !depth || nlist <= 0 || !h->pending.empty()) return -1.0;
    int nsub = 0;
    double t0 = 0;
    for (int i = 0; i < n; i++) {
        if (i == n / 4) { for (auto& c : h->ctx) (void)hipStreamSynchronize(c.stream); (void)hipStreamSynchronize(h->stream); t0 = now_us(); }
        while (nsub < n && !h->ctx[h->open_ctx].launched) {
            if (submit_extract(h, rgb[nsub % nlist], depth[nsub % nlist], 1, nullptr)) return -1.0;
            nsub++;
        }
        if (activate_oldest(h) || retire_active(h)) return -1.0;
        h->stamp++;
    }
    for (auto& c : h->ctx) (void)hipStreamSynchronize(c.stream);
    (void)hipStreamSynchronize(h->stream);
    return (now_us() - t0) / (double)(n - n / 4);
}
// ablation timer for the ICP kernel (tools/icp_probe.py): `reps` back-to-back launches in mode `dbg`
// (bit0: skip the per-surfel math, bit1: skip the LDS accumulation, bit2: skip arrival counting + tail)
double ssf_dbg_time_icp(ssf_handle* h, int reps, int dbg) {
    if (!h || !h->have_frame) return -1.0;
    Rt T; T.R = m3_transpose(h->pose.R); T.t = negate(m3_mulv(T.R, h->pose.t));
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    for (int i = 0; i < 3; i++) launch_icp(h->stream, h->cam, h->model[h->mcur], h->n_visible, h->cc->maps.pix2, h->cc->maps.fpack, T, h->d_icp_replicas, h->d_tickets + 8, h->d_icp, h->mb_dev, ++h->icp_seq, dbg);
    (void)hipEventRecord(e0, h->stream);
    for (int i = 0; i < reps; i++) launch_icp(h->stream, h->cam, h->model[h->mcur], h->n_visible, h->cc->maps.pix2, h->cc->maps.fpack, T, h->d_icp_replicas, h->d_tickets + 8, h->d_icp, h->mb_dev, ++h->icp_seq, dbg);
    (void)hipEventRecord(e1, h->stream);
    (void)hipStreamSynchronize(h->stream);
    float ms = 0.f; (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipMemsetAsync(h->d_icp_replicas, 0, 2 * SSF_ICP_REPLICAS * 32 * sizeof(long long), h->stream);
    (void)hipMemsetAsync(h->d_tickets, 0, 512 * sizeof(unsigned int), h->stream);
    (void)hipStreamSynchronize(h->stream);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 1000.0 * ms / reps;
}
// ablation timer for the fuse launch (tools/fuse_probe.py; lab build; leaves model and partition sums garbage): `reps` back-to-back
// k_update_insert launches on the current frame.  mode bit 0: without the out-of-view arm, bit 1: without update + insert,
// bit 2: without the classification of the visible rows (and then without the update, which needs them)
double ssf_dbg_time_fuse(ssf_handle* h, int reps, int mode, long long* blocks2 /* out-of-view blocks of 256 slots | those with rows that move; may be null */) {
    if (!h || !h->have_frame || !h->cc) return -1.0;
    SurfelSoA& M = h->model[h->mcur];
    PartitionWs ws;
    uint32_t* set = h->d_part + (size_t)h->part_set * h->part_words;
    ws.sup_vis = set; ws.sup_oov = set + h->part_sup_vis; ws.tot = ws.sup_oov + h->part_sup_oov;
    ws.ticket = h->d_part_ticket; ws.other = h->d_part + (size_t)(h->part_set ^ 1) * h->part_words; ws.words = h->part_words;
    const int S = (mode & 2) ? 0 : h->S, nvis = (mode & 4) ? 0 : h->n_visible, span = (mode & 1) ? 0 : h->oov_tail - h->oov_head;
    auto launch = [&] {
        ClassifyArgs ca = h->classify; ca.plane_depth = h->cc->maps.plane_depth;
        launch_fuse(h->stream, M, h->cc->frame, h->pose, h->stamp, h->id_offset, nvis, AssocTables{h->cc->d_best, h->cc->d_matched, h->d_cand, S, 0},
                    (nvis > 0 && S > 0) ? 1 : 0, h->cfg.nb_supersurfels_max, ShardArgs{0, 1, 0, h->cfg.shard_tile}, h->d_cnt,
                    h->oov[h->ocur], span, ca, h->d_state, h->d_state_oov, h->d_bc_oov, ws, 1);
    };
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    for (int i = 0; i < 3 && reps > 0; i++) launch();              // (reps <= 0: only the block census of the last real frame)
    (void)hipEventRecord(e0, h->stream);
    for (int i = 0; i < reps; i++) launch();
    (void)hipEventRecord(e1, h->stream);
    (void)hipStreamSynchronize(h->stream);
    float ms = 0.f; (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (blocks2) {
        const int nb = (span + 255) / 256;
        std::vector<uint32_t> bc((size_t)std::max(nb, 1));
        if (nb > 0) (void)hipMemcpy(bc.data(), h->d_bc_oov, (size_t)nb * 4, hipMemcpyDeviceToHost);
        blocks2[0] = nb; blocks2[1] = 0;
        for (int i = 0; i < nb; i++) blocks2[1] += bc[i] != 0u;
    }
    return reps > 0 ? 1000.0 * ms / reps : 0.0;
}
// one fuse launch on the current frame with every workgroup leaving its three ticks (g_fuse_trace in ssf_track_fuse.hip): out =
// 3 x workgroups words, arms4 = workgroups of update | insertion | visible rows | out-of-view span.  Returns the workgroups, < 0: n/a.
int ssf_dbg_trace_fuse(ssf_handle* h, unsigned long long* out, int cap_wgs, int* arms4, int mode /* as ssf_dbg_time_fuse */) {
    if (!h || !h->have_frame || !h->cc || !out || !arms4) return -1;
    arms4[0] = (mode & 2) ? 0 : (h->S + 31) / 32; arms4[1] = (mode & 2) ? 0 : (h->S + 255) / 256; arms4[2] = (mode & 4) ? 0 : (h->n_visible + 255) / 256;
    long long b2[2];
    unsigned long long* d = nullptr;
    const size_t words = (size_t)3 * 65536;
    if (hipMalloc((void**)&d, words * 8) != hipSuccess) return -2;
    (void)hipMemset(d, 0, words * 8);
    set_fuse_trace(d);
    (void)ssf_dbg_time_fuse(h, 1, mode, b2);         // (3 warm launches with the trace on, then the one whose ticks stay)
    set_fuse_trace(nullptr);
    std::vector<unsigned long long> all(words);
    (void)hipMemcpy(all.data(), d, words * 8, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    int n = 0;
    for (int i = 0; i < 65536; i++) if (all[3 * (size_t)i]) n = i + 1;
    arms4[3] = n - arms4[0] - arms4[1] - arms4[2];
    const int m = n < cap_wgs ? n : cap_wgs;
    std::memcpy(out, all.data(), (size_t)m * 24);
    return m;
}
// the ticks of the move launches (g_move_trace in ssf_track_fuse.hip; tools/move_probe.py).  on: from now on every workgroup of every
// k_move_rows launch leaves eight words -- entry | row and state arrived | prefix known | stores issued | terms in the table | fold
// done | end (100 MHz wall clock; 0: not reached), kind (1 visible, 2 out of view with returning rows, 3 out of view without,
// 4 nothing moves; + 16 a visible block past the last row; + 256 the fused form) -- and a later launch overwrites an earlier one's.
// read: the words of the handle's last move launch, returns the workgroups copied.
static unsigned long long* g_move_trace_words = nullptr;
int ssf_dbg_move_trace(int on) {
    const size_t bytes = (size_t)8 * 65536 * sizeof(unsigned long long);
    if (on && !g_move_trace_words) {
        if (hipMalloc((void**)&g_move_trace_words, bytes) != hipSuccess) return SSF_ERR_INVALID_ARG;
        (void)hipMemset(g_move_trace_words, 0, bytes);
        set_move_trace(g_move_trace_words);
    } else if (!on && g_move_trace_words) {
        (void)hipDeviceSynchronize();
        set_move_trace(nullptr);
        (void)hipFree(g_move_trace_words);
        g_move_trace_words = nullptr;
    }
    return SSF_OK;
}
int ssf_dbg_move_trace_read(ssf_handle* h, unsigned long long* out, int cap_wgs) {
    if (!h || !out || !g_move_trace_words) return -1;
    (void)hipStreamSynchronize(h->stream);
    std::vector<unsigned long long> all((size_t)8 * 65536);
    (void)hipMemcpy(all.data(), g_move_trace_words, all.size() * 8, hipMemcpyDeviceToHost);
    int n = 0;
    for (int i = 0; i < 65536; i++) if (all[8 * (size_t)i]) n = i + 1;
    const int m = n < cap_wgs ? n : cap_wgs;
    std::memcpy(out, all.data(), (size_t)m * 64);
    return m;
}
// the relabelling statistics of the frame just processed (FrameMaps::epoch, SSF_PASS_STAT_* in ssf_extract.hip): out64[8 .. 12];
// collected only after ssf_dbg_pass_stats_enable(1)
int ssf_dbg_pass_stats_enable(int on) { set_pass_stats(on ? 1 : 0); return SSF_OK; }
int ssf_dbg_pass_stats(ssf_handle* h, uint32_t* out64) {
    if (!h || !h->active.ctx || !out64) return SSF_ERR_INVALID_ARG;
    HCK(hipStreamSynchronize(h->active.ctx->stream));
    HCK(hipMemcpy(out64, h->active.maps.epoch, 64 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SSF_OK;
}
// ablation timer for the relabelling pass (tools/pass_probe.py); leaves the segmentation state garbage
double ssf_dbg_time_pass(ssf_handle* h, int reps, int rgbd, int dbg, int nb) {
    if (!h || !h->active.ctx) return -1.0;
    ExtractCtx& c = *h->active.ctx;                   // all slots of the batch context (nb <= extract_batch)
    nb = std::max(1, std::min(nb, h->batch));
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    const int ox[4] = {0, 1, 0, 1}, oy[4] = {0, 1, 1, 0};
    for (int i = 0; i < 4; i++) launch_update_pass(h->stream, h->seg, c.maps, nb, 20 + i, ox[i & 3], oy[i & 3], rgbd != 0, dbg);
    (void)hipEventRecord(e0, h->stream);
    for (int i = 0; i < reps; i++) launch_update_pass(h->stream, h->seg, c.maps, nb, 24 + i, ox[i & 3], oy[i & 3], rgbd != 0, dbg);
    (void)hipEventRecord(e1, h->stream);
    (void)hipStreamSynchronize(h->stream);
    float ms = 0.f; (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 1000.0 * ms / reps;
}
// one pass launch over nb frames of the active context with every workgroup leaving its five ticks (g_pass_trace, ssf_extract.hip);
// `k` = the pass number (>= 20 with rgbd: the frames' state is that of a finished extract, a late pass' workload).  out: 5 words per
// workgroup, grid3 = the launch's grid.  Returns the workgroups copied, < 0: n/a.  Leaves the segmentation state advanced by five passes.
int ssf_dbg_trace_pass(ssf_handle* h, int rgbd, int nb, unsigned long long* out, int cap_wgs, int* grid3) {
    if (!h || !h->active.ctx || !out || !grid3) return -1;
    ExtractCtx& c = *h->active.ctx;
    nb = std::max(1, std::min(nb, h->batch));
    const int ox[4] = {0, 1, 0, 1}, oy[4] = {0, 1, 1, 0};
    grid3[0] = (h->cfg.width + 30 + 31) / 32; grid3[1] = (h->cfg.height + 31) / 32; grid3[2] = nb;
    const int n = grid3[0] * grid3[1] * grid3[2];
    unsigned long long* d = nullptr;
    if (hipMalloc((void**)&d, (size_t)n * 40) != hipSuccess) return -2;
    (void)hipMemset(d, 0, (size_t)n * 40);
    for (int i = 0; i < 4; i++) launch_update_pass(h->stream, h->seg, c.maps, nb, 20 + i, ox[i & 3], oy[i & 3], rgbd != 0, 0);
    (void)hipStreamSynchronize(h->stream);
    set_pass_trace(d);
    launch_update_pass(h->stream, h->seg, c.maps, nb, 24, ox[0], oy[0], rgbd != 0, 0);
    (void)hipStreamSynchronize(h->stream);
    set_pass_trace(nullptr);
    const int m = std::min(n, cap_wgs);
    (void)hipMemcpy(out, d, (size_t)m * 40, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return m;
}
