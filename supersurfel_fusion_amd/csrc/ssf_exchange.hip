// ssf_exchange.hip -- talking to other ranks outside a frame: the RCCL loader, attaching a communicator (ssf_comm_*) or the
// peer-to-peer region (ssf_p2p_*), the shard sizes of all ranks, re-homing a sharded map after a loop closure (ssf_rehome_*).
// The frame path's own exchange calls stay in ssf_host.hip and reach the three functions of ssf_exchange.hpp.
#include <dlfcn.h>
#include "ssf_exchange.hpp"

// ---- RCCL, resolved at run time -------------------------------------------------------------------------
// The multi-GPU exchanges (ssf_comm_attach) call RCCL directly on the track stream.  The symbols come from
// the librccl the process already holds (torch ships one, SONAME librccl.so.1) or from /opt/rocm; a box
// without RCCL still loads libssf_hip.so and runs single-GPU.
RcclApi* rccl_api() {
    static RcclApi api;
    static bool tried = false;
    if (tried) return api.lib ? &api : nullptr;
    tried = true;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) { api.lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD); if (api.lib) break; }   // already in the process?
    if (!api.lib) for (const char* n : names) { api.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (api.lib) break; }
    if (!api.lib) { api.err = "librccl.so.1 not found"; return nullptr; }
    api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(api.lib, "ncclGetUniqueId");
    api.CommInitRank = (decltype(api.CommInitRank))dlsym(api.lib, "ncclCommInitRank");
    api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.lib, "ncclCommDestroy");
    api.AllReduce = (decltype(api.AllReduce))dlsym(api.lib, "ncclAllReduce");
    api.AllGather = (decltype(api.AllGather))dlsym(api.lib, "ncclAllGather");
    api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.lib, "ncclGetErrorString");
    api.CommCount = (decltype(api.CommCount))dlsym(api.lib, "ncclCommCount");
    api.CommUserRank = (decltype(api.CommUserRank))dlsym(api.lib, "ncclCommUserRank");
    api.Broadcast = (decltype(api.Broadcast))dlsym(api.lib, "ncclBroadcast");
    api.CommSplit = (decltype(api.CommSplit))dlsym(api.lib, "ncclCommSplit");
    api.GroupStart = (decltype(api.GroupStart))dlsym(api.lib, "ncclGroupStart");
    api.GroupEnd = (decltype(api.GroupEnd))dlsym(api.lib, "ncclGroupEnd");
    if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.AllReduce || !api.AllGather) {
        api.err = "librccl lacks a required symbol"; api.lib = nullptr; return nullptr;
    }
    return &api;
}

// ---- multi-GPU exchanges (native RCCL on the track stream) -------------------------------------------------
// enqueue the all-gather of every rank's Counters::last and its publication to the mailbox
int comm_gather_counts(ssf_handle* h) {
    const unsigned long long seq = ++h->all_seq;
    if (h->p2p.on) launch_p2p_counts(h->stream, p2p_view(h, ++h->p2p.seq_cnt), h->d_cnt, h->mb_dev, seq);
    else {
        RcclApi* api = rccl_api();
        { ScopedKernel sk("exchange_counts", h->stream);      // (cfg.profile = 1: the collective's time on the track stream, bench.py's exchange_us_per_frame)
          NCK(api->AllGather(h->d_cnt->last, h->d_all5, 5, ncclInt32, h->comm, h->stream)); }
        launch_publish_all_counts(h->stream, h->d_all5, h->cfg.nranks, h->mb_dev, seq);
    }
    HCK(hipGetLastError());
    h->all_pending = true;
    return SSF_OK;
}
// the shard sizes of all ranks after the previous frame -> global counts and this shard's id offset
int comm_counts(ssf_handle* h) {
    if (!h->all_valid && !h->all_pending) { int rc = comm_gather_counts(h); if (rc) return rc; }
    if (h->all_pending) {
        int rc = wait_seq(h, &h->mb_host->all_seq, h->all_seq);
        if (rc) return rc;
        const int n = 5 * h->cfg.nranks;
        int w[MAILBOX_SHARD_WORDS];
        for (int attempt = 0; !int_record_read(h->mb_host->all_cnt, n, &h->mb_host->all_check, h->all_seq, w); attempt++)
            if (attempt > 100000) { h->err = "shard-size mailbox record failed its checksum"; return SSF_ERR_DEVICE; }
        for (int i = 0; i < n; i++) h->all_cnt[i] = w[i];
        h->all_pending = false; h->all_valid = true;
    }
    long long gm = 0, gv = 0, off = 0;
    for (int r = 0; r < h->cfg.nranks; r++) {
        gm += h->all_cnt[5 * r]; gv += h->all_cnt[5 * r + 1];
        if (r < h->cfg.rank) off += h->all_cnt[5 * r + 1];
    }
    h->global_n_model = gm; h->global_n_visible = gv; h->id_offset = off;
    return SSF_OK;
}

extern "C" {
// ---- multi-GPU (native RCCL) ------------------------------------------------------------------------------
int ssf_comm_unique_id(uint8_t* id128) {
    if (!id128) return SSF_ERR_INVALID_ARG;
    RcclApi* api = rccl_api();
    if (!api) { set_create_error("RCCL is not available in this process"); return SSF_ERR_DEVICE; }
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId id;
    if (api->GetUniqueId(&id) != ncclSuccess) { set_create_error("ncclGetUniqueId failed"); return SSF_ERR_DEVICE; }
    std::memcpy(id128, &id, 128);
    return SSF_OK;
}
int ssf_comm_attach(ssf_handle* h, const uint8_t* id128) {
    if (!h || !id128) return SSF_ERR_INVALID_ARG;
    if (h->comm) { h->err = "a communicator is already attached"; return SSF_ERR_STATE; }
    if (h->cfg.nranks > SSF_MAX_RANKS) { h->err = "too many ranks"; return SSF_ERR_INVALID_ARG; }
    RcclApi* api = rccl_api();
    if (!api) { h->err = "RCCL is not available in this process"; return SSF_ERR_DEVICE; }
    HCK(hipSetDevice(h->cfg.device_id));
    if (!h->d_all5 && !dalloc(h, &h->d_all5, 5 * SSF_MAX_RANKS)) { h->err = "allocation failed"; return SSF_ERR_DEVICE; }
    ncclUniqueId id;
    std::memcpy(&id, id128, 128);
    NCK(api->CommInitRank(&h->comm, h->cfg.nranks, id, h->cfg.rank));
    drop_shard_sizes(h);
    return SSF_OK;
}
// The extract stage dealt over the ranks (see launch_batch): one communicator per batch context, split off the attached one --
// a collective call, made by every rank after ssf_comm_attach and with an empty pipeline.  mode 0: back to the replicated form.
int ssf_comm_deal_extract(ssf_handle* h, int mode) {
    if (!h || mode < 0 || mode > 2) return SSF_ERR_INVALID_ARG;
    if (!h->comm) { h->err = "ssf_comm_deal_extract: attach an RCCL communicator first (the peer-to-peer backend keeps the extract stage replicated)"; return SSF_ERR_STATE; }
    if (!h->pending.empty()) { h->err = "frames are pending in the extract pipeline"; return SSF_ERR_STATE; }
    for (auto& c : h->ctx) if (c.count > 0 || c.launched) { h->err = "a batch is open in the extract pipeline"; return SSF_ERR_STATE; }
    RcclApi* api = rccl_api();
    if (!api || !api->Broadcast || !api->CommSplit || !api->GroupStart || !api->GroupEnd) { h->err = "this RCCL has no ncclCommSplit / ncclBroadcast"; return SSF_ERR_DEVICE; }
    HCK(hipSetDevice(h->cfg.device_id));
    if (mode != 0)
        for (auto& c : h->ctx)
            if (!c.deal_comm) NCK(api->CommSplit(h->comm, 0, h->cfg.rank, &c.deal_comm, nullptr));
    h->deal = mode; h->deal_batches = 0;
    return SSF_OK;
}
int ssf_comm_info(ssf_handle* h, int* backend, int* ranks, int* my_rank) {
    if (!h) return SSF_ERR_INVALID_ARG;
    int b = 0, n = 1, r = 0;
    if (h->comm) {
        b = 1; n = h->cfg.nranks; r = h->cfg.rank;
        RcclApi* api = rccl_api();
        if (api && api->CommCount && api->CommUserRank) { NCK(api->CommCount(h->comm, &n)); NCK(api->CommUserRank(h->comm, &r)); }
    } else if (h->p2p.on) {
        b = 2; n = (int)h->p2p.opened.size() + 1; r = h->cfg.rank;
        if (h->p2p.opened.empty()) n = h->cfg.nranks;        // ranks of one process (ssf_p2p_attach_local): nothing was opened through IPC
    }
    if (backend) *backend = b;
    if (ranks) *ranks = n;
    if (my_rank) *my_rank = r;
    return SSF_OK;
}
// ---- multi-GPU (native, peer to peer: no collective launches) ---------------------------------------------------
// the bound of every in-kernel wait for a peer, in ticks of the device's constant-rate wall clock (wall_clock64)
static int p2p_set_timeout(ssf_handle* h) {
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->cfg.device_id) != hipSuccess || khz <= 0) { (void)hipGetLastError(); khz = 100000; }
    h->p2p.view.timeout_ticks = (unsigned long long)(h->p2p.timeout_s * 1000.0 * (double)khz);
    return SSF_OK;
}
static int p2p_region(ssf_handle* h) {
    if (h->p2p.region) return SSF_OK;
    if (h->cfg.nranks > SSF_P2P_MAX_RANKS) { h->err = "the peer-to-peer exchange serves at most 8 ranks (one node)"; return SSF_ERR_INVALID_ARG; }
    HCK(hipSetDevice(h->cfg.device_id));
    const size_t bytes = p2p_region_bytes(h->S);
    void* q = nullptr;
    // Which memory: peers store into this region and this rank's kernels poll it WHILE THEY RUN.  HIP guarantees coherence
    // of ordinary (coarse-grained) device memory across devices only at kernel boundaries -- the owner's L2 may serve its
    // polling loads stale lines while another GPU writes over xGMI -- so the region is FINE-GRAINED device memory
    // (hipDeviceMallocFinegrained) unless the caller has declared, through ssf_p2p_configure, that every rank of the map
    // lives on this handle's device (several shards on one GPU: the one arrangement this build could be run in).  There
    // plain memory is used: all accesses to a region are system-scope atomics that meet in the same memory, and round 2's
    // campaigns (profiles/p2p_campaigns_r02.txt) ran 2600 create-attach-run cycles clean with it against 211 bad ones with
    // an UNCACHED region (hipDeviceMallocUncached; SSF_P2P_REGION_UNCACHED=1 brings that mapping back for experiments).
    static const bool uncached = SSF_ENV_SET("P2P_REGION_UNCACHED");
    if (uncached && hipExtMallocWithFlags(&q, bytes, hipDeviceMallocUncached) == hipSuccess) h->p2p.fine = true;
    else if (!uncached && !h->p2p.same_device && hipExtMallocWithFlags(&q, bytes, hipDeviceMallocFinegrained) == hipSuccess) h->p2p.fine = true;
    else {
        (void)hipGetLastError();
        if (!h->p2p.same_device && !uncached) { h->err = "fine-grained device memory for the exchange region is not available"; return SSF_ERR_DEVICE; }
        HCK(hipMalloc(&q, bytes));
    }
    HCK(hipMemset(q, 0, bytes));
    HCK(hipDeviceSynchronize());
    h->p2p.region = (unsigned char*)q; h->p2p.bytes = bytes;
    return SSF_OK;
}
int ssf_p2p_configure(ssf_handle* h, int all_ranks_on_this_device, double timeout_s) {
    if (!h || !(timeout_s > 0.0)) return SSF_ERR_INVALID_ARG;
    if (h->p2p.region && (all_ranks_on_this_device != 0) != h->p2p.same_device) {
        h->err = "ssf_p2p_configure: the exchange region is already allocated (call before ssf_p2p_export / ssf_p2p_region)"; return SSF_ERR_STATE;
    }
    h->p2p.same_device = all_ranks_on_this_device != 0;
    h->p2p.timeout_s = timeout_s;
    if (h->p2p.on) { int rc = p2p_set_timeout(h); if (rc) return rc; }
    return SSF_OK;
}
int ssf_p2p_region(ssf_handle* h, void** region, size_t* bytes) {
    if (!h || !region) return SSF_ERR_INVALID_ARG;
    int rc = p2p_region(h);
    if (rc) return rc;
    *region = h->p2p.region; if (bytes) *bytes = h->p2p.bytes;
    return SSF_OK;
}
int ssf_p2p_export(ssf_handle* h, uint8_t* handle64) {
    if (!h || !handle64) return SSF_ERR_INVALID_ARG;
    int rc = p2p_region(h);
    if (rc) return rc;
    static_assert(sizeof(hipIpcMemHandle_t) == SSF_P2P_HANDLE_BYTES, "hipIpcMemHandle_t is 64 bytes");
    hipIpcMemHandle_t ih;
    HCK(hipIpcGetMemHandle(&ih, h->p2p.region));
    std::memcpy(handle64, &ih, sizeof(ih));
    return SSF_OK;
}
static int p2p_finish_attach(ssf_handle* h) {
    { int rc = p2p_set_timeout(h); if (rc) return rc; }
    h->p2p.view.me = h->cfg.rank; h->p2p.view.nranks = h->cfg.nranks; h->p2p.view.S = h->S; h->p2p.view.seq = 0;
    h->p2p.on = true;
    drop_shard_sizes(h);
    return SSF_OK;
}
static int p2p_attach_check(ssf_handle* h) {
    if (h->comm || h->p2p.on) { h->err = "an exchange backend is already attached"; return SSF_ERR_STATE; }
    if (h->stamp != 0 && h->cfg.nranks > 1) { /* joining later is fine as long as every rank does so at the same frame */ }
    return p2p_region(h);
}
int ssf_p2p_attach(ssf_handle* h, const uint8_t* handles) {
    if (!h || !handles) return SSF_ERR_INVALID_ARG;
    int rc = p2p_attach_check(h);
    if (rc) return rc;
    for (int r = 0; r < h->cfg.nranks; r++) {
        if (r == h->cfg.rank) { h->p2p.view.peer[r] = h->p2p.region; continue; }
        hipIpcMemHandle_t ih;
        std::memcpy(&ih, handles + (size_t)SSF_P2P_HANDLE_BYTES * r, sizeof(ih));
        void* q = nullptr;
        HCK(hipIpcOpenMemHandle(&q, ih, hipIpcMemLazyEnablePeerAccess));
        h->p2p.opened.push_back(q);
        h->p2p.view.peer[r] = (unsigned char*)q;
    }
    return p2p_finish_attach(h);
}
int ssf_p2p_attach_local(ssf_handle* h, void* const* regions) {
    if (!h || !regions) return SSF_ERR_INVALID_ARG;
    int rc = p2p_attach_check(h);
    if (rc) return rc;
    for (int r = 0; r < h->cfg.nranks; r++) {
        if (r != h->cfg.rank && !regions[r]) { h->err = "a peer region is missing"; return SSF_ERR_INVALID_ARG; }
        h->p2p.view.peer[r] = r == h->cfg.rank ? h->p2p.region : (unsigned char*)regions[r];
    }
    return p2p_finish_attach(h);
}
int ssf_get_global_counts(ssf_handle* h, int64_t* out5) {
    if (!h || !out5) return SSF_ERR_INVALID_ARG;
    if (!h->comm && !h->p2p.on) {
        int rc = hipStreamSynchronize(h->stream) == hipSuccess ? SSF_OK : SSF_ERR_DEVICE;
        Counters c;
        if (rc || hipMemcpy(&c, h->d_cnt, sizeof(c), hipMemcpyDeviceToHost) != hipSuccess) { h->err = "device error"; return SSF_ERR_DEVICE; }
        for (int i = 0; i < 5; i++) out5[i] = c.last[i];
        return SSF_OK;
    }
    int rc = comm_counts(h);
    if (rc) return rc;
    for (int i = 0; i < 5; i++) { out5[i] = 0; for (int r = 0; r < h->cfg.nranks; r++) out5[i] += h->all_cnt[5 * r + i]; }
    return SSF_OK;
}

// ---- re-homing of a sharded map (see ssf.h): rows moved by ssf_apply_deformation go to the rank that owns their tile ----
// A rare, bulk operation (a loop closure): worked on the dense logical view with full-model copies; the transport between
// the ranks is the caller's (supersurfel_fusion_amd/sharded.py: torch.distributed; the tests: files / memory).
int ssf_rehome_begin(ssf_handle* h, int32_t* table, int table_rows, int* n_out) {
    if (!h || !n_out || table_rows < 0 || (!table && table_rows > 0)) return SSF_ERR_INVALID_ARG;
    { int rc = model_at_rest(h); if (rc) return rc; }
    *n_out = 0;
    drop_shard_sizes(h);
    const int n = h->n_model;
    if (h->cfg.nranks <= 1 || n == 0) return SSF_OK;
    hipStream_t st = h->stream;
    { int rc = materialise(h); if (rc) return rc; }
    int32_t* d_table = nullptr; int* d_tot = nullptr;
    DevTemps tmp;
    HCK(tmp.take(&d_table, (size_t)std::max(table_rows, 1) * SSF_MIGRANT_WORDS * 4)); HCK(tmp.take(&d_tot, 16));
    SurfelSoA scratch = h->oov[h->ocur ^ 1].rows;          // (the other out-of-view store is scratch between recentres)
    launch_rehome_split(st, h->dense, n, h->n_visible, h->cfg.rank, h->cfg.nranks, h->cfg.shard_tile, h->d_bc_oov, d_tot, scratch, d_table, table_rows);
    HCK(hipGetLastError());
    int tot[3] = {0, 0, 0};
    HCK(hipMemcpyAsync(tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, st));
    HCK(hipStreamSynchronize(st));
    if (tot[1] > table_rows) { h->err = "ssf_rehome_begin: the table is too small for the rows that leave"; return SSF_ERR_CAPACITY; }   // (stores untouched)
    if (tot[1] == 0) return SSF_OK;
    HCK(hipMemcpyAsync(table, d_table, (size_t)tot[1] * SSF_MIGRANT_WORDS * 4, hipMemcpyDeviceToHost, st));
    { int rc = copy_soa(h, h->dense, scratch, (size_t)tot[0]); if (rc) return rc; }
    { int rc = store_from_dense(h, tot[0], tot[2]); if (rc) return rc; }
    HCK(hipStreamSynchronize(st));
    *n_out = tot[1];
    return SSF_OK;
}
int ssf_rehome_end(ssf_handle* h, const int32_t* table, int n_rec) {
    if (!h || n_rec < 0 || (!table && n_rec > 0)) return SSF_ERR_INVALID_ARG;
    { int rc = model_at_rest(h); if (rc) return rc; }
    drop_shard_sizes(h);
    // the records addressed to this rank, split by the block they arrive in (table order kept).  A full shard turns the
    // surplus away, in table order, as a frame's migration does (k_migrate_in): their source shards have already let them
    // go, so they are lost to the map -- the call still succeeds on every rank (an error here would leave the ranks in
    // different states with nothing to roll back) and returns their number
    std::vector<int32_t> vis, oov;
    const int n = h->n_model, nv = h->n_visible;
    int room = h->cfg.nb_supersurfels_max - n, turned_away = 0;
    for (int j = 0; j < n_rec; j++) {
        const int32_t* w = table + (size_t)SSF_MIGRANT_WORDS * j;
        if (w[0] - 1 != h->cfg.rank) continue;
        if (room <= 0) { turned_away++; continue; }
        room--;
        std::vector<int32_t>& dst = w[1] ? vis : oov;
        dst.insert(dst.end(), w, w + SSF_MIGRANT_WORDS);
    }
    const int av = (int)(vis.size() / SSF_MIGRANT_WORDS), ao = (int)(oov.size() / SSF_MIGRANT_WORDS);
    if (av + ao == 0) return turned_away;
    hipStream_t st = h->stream;
    { int rc = materialise(h); if (rc) return rc; }
    int32_t* d_rec = nullptr;
    DevTemps tmp;
    HCK(tmp.take(&d_rec, (size_t)(av + ao) * SSF_MIGRANT_WORDS * 4));
    if (av) HCK(hipMemcpyAsync(d_rec, vis.data(), vis.size() * 4, hipMemcpyHostToDevice, st));
    if (ao) HCK(hipMemcpyAsync(d_rec + vis.size(), oov.data(), oov.size() * 4, hipMemcpyHostToDevice, st));
    // [visible | arrivals flagged visible | out of view | the other arrivals], assembled in the scratch store
    SurfelSoA scratch = h->oov[h->ocur ^ 1].rows;
    { int rc = copy_soa(h, scratch, h->dense, (size_t)nv); if (rc) return rc; }
    launch_rehome_unpack(st, d_rec, av, scratch, nv);
    { int rc = copy_soa(h, soa_rows(scratch, (size_t)nv + av), soa_rows(h->dense, (size_t)nv), (size_t)(n - nv)); if (rc) return rc; }
    launch_rehome_unpack(st, d_rec + vis.size(), ao, scratch, n + av);
    HCK(hipGetLastError());
    { int rc = copy_soa(h, h->dense, scratch, (size_t)n + av + ao); if (rc) return rc; }
    { int rc = store_from_dense(h, n + av + ao, nv + av); if (rc) return rc; }
    HCK(hipStreamSynchronize(st));
    return turned_away;
}
}  // extern "C"
