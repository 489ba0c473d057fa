// Included by engine.hip inside its `extern "C"` block: the communicator (SURVEY.md section 8e); the sharded drivers are in comm_api.inc / tipa_api.inc.
//
// One process per GPU.  Vectors are sharded by index residue (element i on rank i mod G), so every halving round folds locally and the
// only exchange is the rank's partial GT products (2 x 576 B per SIPP round): RCCL has no Fq12-product reduction, hence
// ALL-GATHER + local multiply.  The collective lives HERE, behind the C ABI, so that a Rust host binds one call
// (`ripp_sipp_prove_sharded`) instead of re-implementing the round loop:
//   * transport "rccl": librccl.so is dlopen'ed on first use (ncclAllGather on the engine's stream; xGMI between the GPUs of a node);
//     the 128-byte ncclUniqueId is created by rank 0 (`ripp_comm_unique_id`) and handed to the other ranks by the HOST -- the host
//     already has a rendezvous (torch.distributed store, MPI, a file), the library does not invent another one;
//   * transport "callback": the host supplies an all-gather function (used by the world-2 tests on one GPU / on CPU boxes over gloo).
extern "C++" {
#include <dlfcn.h>
#include <rccl/rccl.h>
namespace {
inline void cpu_relax() {
#if defined(__x86_64__)
    __builtin_ia32_pause();
#else
    std::this_thread::yield();
#endif
}
struct Comm {
    int rank = 0, world = 1;
    bool active = false;
    // callback transport
    ripp_allgather_fn cb = nullptr; void* cb_user = nullptr;
    // RCCL transport
    void* dl = nullptr; ncclComm_t nccl = nullptr;
    ncclResult_t (*pGetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*pCommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*pAllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*pCommDestroy)(ncclComm_t) = nullptr;
    const char* (*pGetErrorString)(ncclResult_t) = nullptr;
    DevBuf send, recv;
    PinBuf hsend, hrecv;             // pinned staging: the copies around the collective are plain DMA on the communicator's stream, one synchronisation per exchange
    hipStream_t st = nullptr;        // own stream: an exchange never queues behind folds / products the prover has enqueued on the engine's streams
    bool replay = false;             // transport "replay": the peers' blocks come from a recording (below)
    ncclResult_t (*pCommAbort)(ncclComm_t) = nullptr;
    uint64_t n_ex = 0;               // exchanges since the communicator was brought up (error messages name the one that failed)
    bool broken = false;             // an exchange ran into its deadline: a collective of a dead or absent peer is still queued on `st`; nothing more can be issued
};
Comm g_comm;

// ---- the ranks of ONE process (ripp_config.n_devices > 1 on a fused prover: tipa_api.inc) ------------------------------------------------------------------
// D host threads, one per device, walk the sharded protocol of a proof side by side; their "all-gather" is a copy through this object -- no RCCL, no host
// rendezvous.  Two slabs alternate by exchange number: a thread reads slab k before it can enter exchange k + 1, and nobody writes slab k again before
// exchange k + 2, which needs everybody through k + 1.  A thread that leaves with an error fails the group: the others return at (or inside) their next exchange.
struct LocalComm {
    int world = 1;
    std::mutex m; std::condition_variable cv;
    uint64_t gen = 0; int arrived = 0; size_t bytes = 0; bool failed = false;
    std::vector<uint8_t> slab[2];
    void fail() { { std::lock_guard<std::mutex> lk(m); failed = true; } cv.notify_all(); }
};
thread_local LocalComm* t_lcomm = nullptr; thread_local int t_lrank = 0;
int32_t local_allgather(const void* send, void* recv, size_t bytes) {
    LocalComm& lc = *t_lcomm;
    std::unique_lock<std::mutex> lk(lc.m);
    if (lc.failed) { set_err("in-process ranks: another device's prover failed"); return RIPP_ERR_DEVICE; }
    const uint64_t my = lc.gen; std::vector<uint8_t>& sb = lc.slab[my & 1];
    if (lc.arrived == 0) { lc.bytes = bytes; sb.resize(bytes * (size_t)lc.world); }
    else if (lc.bytes != bytes) { lc.failed = true; lk.unlock(); lc.cv.notify_all(); set_err("in-process ranks: the devices' provers disagree on the size of an exchange"); return RIPP_ERR_ARG; }
    std::memcpy(sb.data() + (size_t)t_lrank * bytes, send, bytes);
    if (++lc.arrived == lc.world) { lc.arrived = 0; ++lc.gen; lk.unlock(); lc.cv.notify_all(); lk.lock(); }
    else lc.cv.wait(lk, [&]() { return lc.gen != my || lc.failed; });
    if (lc.gen == my) { set_err("in-process ranks: another device's prover failed"); return RIPP_ERR_DEVICE; }      // (woken by a failure, not by the exchange)
    std::memcpy(recv, sb.data(), bytes * (size_t)lc.world);
    return RIPP_OK;
}

// ---- recorded peers (transport "replay") -----------------------------------------------------------------------------------------------
// A proof is deterministic, so the blocks a rank receives in its all-gathers are too.  A RECORDING holds the exchanges of one proof: per
// exchange the gathered blocks of all ranks and, per rank, the GAP between the completion of the previous exchange (the start of the proof
// for the first one) and the rank's arrival at this one -- the rank's own work on the critical path, NaN where nobody has measured it.
// Recording: any live communicator, `ripp_comm_record(1)` (the 2/4/8 processes of the one-device rig produce the blocks; their gaps are
// time-sliced and are not kept).  Replay: ONE process is rank k of G, alone on the device and therefore at full speed; an all-gather
// returns the recorded blocks with the caller's own block in its slot, no earlier than the slowest peer whose gaps are known would have
// arrived (previous completion + its gap) plus a fixed latency -- a discrete-event model of the G-rank run in which this rank is live.
// The rank's own gaps and blocks are written back (`ripp_comm_recording_save`), so that rank 0's solo pass gives the other ranks their
// deadline (its plan message, its digest time) and a second pass of rank 0 sees the measured peers.  tools/replay_ranks.py drives it.
// What an exchanged block is made of -- for the REPLAY's check of the live rank's own block against the recorded one.  Most messages are byte-deterministic
// (finished GT values, affine points, transcripts); three are not, legitimately: the plan message carries clock readings; a Miller value before the final
// exponentiation is only defined up to a factor of a proper subfield (it depends on how the launch was cut, i.e. on free memory and batch sizes); a partial MSM
// sum is a projective point whose representative depends on the summation order.  Those are compared for what they MEAN (deferred to ripp_comm_replay_check:
// a final exponentiation per differing value costs ~1 ms and must not sit inside a timed exchange); everything else must match byte for byte.
enum ExKind : uint8_t { EX_RAW = 0, EX_PLAN = 1, EX_GT = 2, EX_G1J = 3, EX_G2J = 4 };
thread_local uint8_t t_ex_kind = EX_RAW;                 // set by the sender right before comm_allgather, consumed by it
struct ExDesc { uint8_t k0 = EX_RAW, k1 = EX_RAW; uint32_t b0 = 0, b1 = 0; bool mux = false; };      // mux: an 8-byte header, then block0 (b0 bytes, kind k0), then block1
thread_local ExDesc t_ex_desc;
struct Recording {
    struct Ex { uint32_t bytes = 0; std::vector<double> gap; std::vector<uint8_t> data; };
    struct Differing { size_t ex; ExDesc d; std::vector<uint8_t> live, rec; };
    std::vector<Differing> differing;                    // own blocks whose bytes differed from the recording, kept for the semantic check
    uint64_t mismatches = 0; std::string first_mismatch;
    std::vector<Ex> ex;
    int world = 0;
    bool recording = false, marked = false;
    size_t cur = 0;
    double t_prev = 0, latency_ms = 0;
    uint64_t served = 0, own_differs = 0; double waited_ms = 0;
};
Recording g_rec;
// start of a proof (every sharded driver calls it on entry; of nested calls the outermost wins: `marked` = "marked, and no exchange since"):
// a recording restarts -- it holds the exchanges since the LAST mark --, a replay rewinds
void comm_mark_proof() {
    if (!g_rec.recording && !g_comm.replay) return;
    if (g_rec.marked) return;
    g_rec.marked = true; g_rec.t_prev = now_ms(); g_rec.cur = 0;
    if (g_rec.recording) g_rec.ex.clear();
}
int32_t replay_allgather(const void* send, void* recv, size_t bytes) {
    const double t_in = now_ms();
    if (g_rec.cur >= g_rec.ex.size()) { set_err("replay: exchange " + std::to_string(g_rec.cur) + " is beyond the recording (" + std::to_string(g_rec.ex.size()) + " exchanges)"); return RIPP_ERR_ARG; }
    Recording::Ex& x = g_rec.ex[g_rec.cur];
    if (x.bytes != bytes) { set_err("replay: exchange " + std::to_string(g_rec.cur) + " carries " + std::to_string(bytes) + " bytes per rank, the recording has " + std::to_string(x.bytes)); return RIPP_ERR_ARG; }
    double ready = t_in;
    for (int r = 0; r < g_comm.world; ++r) if (r != g_comm.rank && x.gap[r] == x.gap[r]) ready = std::max(ready, g_rec.t_prev + x.gap[r]);
    ready += g_rec.latency_ms;
    while (now_ms() < ready) cpu_relax();
    uint8_t* own = x.data.data() + (size_t)g_comm.rank * bytes;
    if (std::memcmp(own, send, bytes)) {
        ++g_rec.own_differs;
        g_rec.differing.push_back({g_rec.cur, t_ex_desc, std::vector<uint8_t>(static_cast<const uint8_t*>(send), static_cast<const uint8_t*>(send) + bytes), std::vector<uint8_t>(own, own + bytes)});
        std::memcpy(own, send, bytes);
    }
    std::memcpy(recv, x.data.data(), bytes * (size_t)g_comm.world);
    x.gap[g_comm.rank] = t_in - g_rec.t_prev;
    const double t_out = now_ms();
    g_rec.waited_ms += t_out - t_in; ++g_rec.served; ++g_rec.cur; g_rec.t_prev = t_out; g_rec.marked = false;
    return RIPP_OK;
}
void record_exchange(const void* recv, size_t bytes, double t_in) {
    Recording::Ex x; x.bytes = (uint32_t)bytes; x.gap.assign((size_t)g_comm.world, __builtin_nan(""));
    x.gap[g_comm.rank] = t_in - g_rec.t_prev;
    x.data.assign(static_cast<const uint8_t*>(recv), static_cast<const uint8_t*>(recv) + bytes * (size_t)g_comm.world);
    g_rec.ex.push_back(std::move(x)); g_rec.world = g_comm.world; g_rec.t_prev = now_ms(); g_rec.marked = false;
}

int32_t rccl_load() {
    if (g_comm.dl) return RIPP_OK;
    // RCCL must sit on the SAME HIP runtime this library is bound to.  A process may hold two ROCm installations (a PyTorch wheel bundles its
    // own libamdhip64 / librccl next to /opt/rocm's), and a bare dlopen("librccl.so.1") returns whichever copy was loaded first -- a
    // communicator created on the other runtime fails with "unhandled cuda error".  So: look beside the libamdhip64 actually in use.
    void* h = nullptr;
    {
        Dl_info info;
        if (dladdr(reinterpret_cast<void*>(&hipGetDeviceCount), &info) && info.dli_fname) {
            std::string dir(info.dli_fname); const size_t slash = dir.rfind('/');
            if (slash != std::string::npos) {
                dir.resize(slash + 1);
                for (const char* name : {"librccl.so.1", "librccl.so"}) { h = dlopen((dir + name).c_str(), RTLD_NOW | RTLD_LOCAL); if (h) break; }
            }
        }
    }
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) { set_err(std::string("cannot load librccl.so: ") + dlerror()); return RIPP_ERR_DEVICE; }
    g_comm.pGetUniqueId = reinterpret_cast<decltype(g_comm.pGetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
    g_comm.pCommInitRank = reinterpret_cast<decltype(g_comm.pCommInitRank)>(dlsym(h, "ncclCommInitRank"));
    g_comm.pAllGather = reinterpret_cast<decltype(g_comm.pAllGather)>(dlsym(h, "ncclAllGather"));
    g_comm.pCommDestroy = reinterpret_cast<decltype(g_comm.pCommDestroy)>(dlsym(h, "ncclCommDestroy"));
    g_comm.pGetErrorString = reinterpret_cast<decltype(g_comm.pGetErrorString)>(dlsym(h, "ncclGetErrorString"));
    g_comm.pCommAbort = reinterpret_cast<decltype(g_comm.pCommAbort)>(dlsym(h, "ncclCommAbort"));
    if (!g_comm.pGetUniqueId || !g_comm.pCommInitRank || !g_comm.pAllGather || !g_comm.pCommDestroy) { set_err("librccl.so lacks an expected symbol"); dlclose(h); return RIPP_ERR_DEVICE; }
    g_comm.dl = h; return RIPP_OK;
}
#define NCCLCHK(expr) do { ncclResult_t r_ = (expr); if (r_ != ncclSuccess) { set_err(std::string(#expr) + ": " + (g_comm.pGetErrorString ? g_comm.pGetErrorString(r_) : "rccl error")); return RIPP_ERR_DEVICE; } } while (0)

// all-gather of `bytes` host bytes per rank into recv[world][bytes] (rank order); world == 1 copies
int32_t comm_allgather_live(Engine* e, const void* send, void* recv, size_t bytes);
int32_t comm_allgather_one(Engine* e, const void* send, void* recv, size_t bytes);
// ---- two provers of one call on one communicator (sharded aggregate_proofs: the TIPP and the TIPAWithSSM sub-proofs side by side) ---------------------
// The ranks' collectives must be issued in ONE agreed order, and two host threads that reach their exchanges whenever their devices are done would not
// agree on one.  CommMux pairs them by COUNT instead: the k-th exchange of channel 0 and the k-th exchange of channel 1 travel in ONE all-gather
// ([bytes0, bytes1, block0, block1] per rank), issued by whichever thread arrives second; once a channel has declared itself done, the other one's
// exchanges travel alone.  Every sub-proof makes the same number of exchanges on every rank (rounds, tail gather, KZG openings), so the composition of
// every all-gather is the same on every rank whatever the threads' timing -- and a round costs one exchange, not two.  A channel that ends with an
// error makes the other channel's next exchange fail at once, without entering the collective (the rank leaves the protocol, as any failing rank of a
// sharded GIPA / TIPA proof does).
struct CommMux {
    std::mutex m; std::condition_variable cv;
    bool active = false;
    struct Chan { bool posted = false, done = false; const void* send = nullptr; void* recv = nullptr; size_t bytes = 0; int32_t rc = 0, done_rc = 0; uint64_t served = 0; std::string err; uint8_t kind = 0; } ch[2];      // err: the message that goes with rc (g_err is thread-local: the waiter sets it on its own thread)
    std::vector<uint8_t> frame, all;
};
CommMux g_mux;
thread_local int t_mux_chan = -1;
void mux_begin() { std::lock_guard<std::mutex> lk(g_mux.m); g_mux.ch[0] = CommMux::Chan(); g_mux.ch[1] = CommMux::Chan(); g_mux.active = true; }
void mux_end() { std::lock_guard<std::mutex> lk(g_mux.m); g_mux.active = false; }
void mux_done(int c, int32_t rc) { { std::lock_guard<std::mutex> lk(g_mux.m); g_mux.ch[c].done = true; g_mux.ch[c].done_rc = rc; } g_mux.cv.notify_all(); }
int32_t mux_allgather(Engine* e, int c, const void* send, void* recv, size_t bytes, uint8_t kind) {
    std::unique_lock<std::mutex> lk(g_mux.m);
    CommMux::Chan& me = g_mux.ch[c]; CommMux::Chan& other = g_mux.ch[1 - c];
    me.posted = true; me.send = send; me.recv = recv; me.bytes = bytes; me.kind = kind;
    const uint64_t ticket = me.served;
    if (!other.posted && !other.done) {
        g_mux.cv.wait(lk, [&]() { return me.served != ticket || other.posted || other.done; });
        if (me.served != ticket) { if (me.rc) set_err(me.err); return me.rc; }      // the other thread carried this block with its own
    }
    if (other.done && other.done_rc) { me.posted = false; set_err("sharded aggregate_proofs: the other sub-proof of this rank failed"); return RIPP_ERR_DEVICE; }
    const int world = g_comm.world;
    const size_t b0 = g_mux.ch[0].posted ? g_mux.ch[0].bytes : 0, b1 = g_mux.ch[1].posted ? g_mux.ch[1].bytes : 0, fsz = 8 + b0 + b1;
    g_mux.frame.resize(fsz); g_mux.all.resize(fsz * (size_t)world);
    const uint32_t hdr[2] = {(uint32_t)b0, (uint32_t)b1};
    std::memcpy(g_mux.frame.data(), hdr, 8);
    if (b0) std::memcpy(g_mux.frame.data() + 8, g_mux.ch[0].send, b0);
    if (b1) std::memcpy(g_mux.frame.data() + 8 + b0, g_mux.ch[1].send, b1);
    t_ex_desc = ExDesc{g_mux.ch[0].kind, g_mux.ch[1].kind, (uint32_t)b0, (uint32_t)b1, true};
    int32_t rc = comm_allgather_one(e, g_mux.frame.data(), g_mux.all.data(), fsz);
    for (int w = 0; w < world && !rc; ++w) {
        const uint8_t* f = g_mux.all.data() + (size_t)w * fsz;
        if (std::memcmp(f, hdr, 8)) { set_err("sharded aggregate_proofs: rank " + std::to_string(w) + " paired its sub-proofs' exchanges differently"); rc = RIPP_ERR_ARG; break; }
        if (b0) std::memcpy(static_cast<uint8_t*>(g_mux.ch[0].recv) + (size_t)w * b0, f + 8, b0);
        if (b1) std::memcpy(static_cast<uint8_t*>(g_mux.ch[1].recv) + (size_t)w * b1, f + 8 + b0, b1);
    }
    for (CommMux::Chan& ch : g_mux.ch) if (ch.posted) { ch.posted = false; ch.rc = rc; if (rc) ch.err = ripp_last_error(); ++ch.served; }
    lk.unlock(); g_mux.cv.notify_all();
    return rc;
}
int32_t comm_allgather(Engine* e, const void* send, void* recv, size_t bytes) {
    const uint8_t kind = t_ex_kind; t_ex_kind = EX_RAW;
    if (t_lcomm) return local_allgather(send, recv, bytes);            // this thread is one of the in-process ranks of a fused prover
    if (!g_comm.active || g_comm.world == 1) { std::memcpy(recv, send, bytes); return RIPP_OK; }
    if (g_mux.active && t_mux_chan >= 0) return mux_allgather(e, t_mux_chan, send, recv, bytes, kind);
    t_ex_desc = ExDesc{kind, EX_RAW, (uint32_t)bytes, 0, false};
    return comm_allgather_one(e, send, recv, bytes);
}
int32_t comm_allgather_one(Engine* e, const void* send, void* recv, size_t bytes) {
    if (g_comm.replay) return replay_allgather(send, recv, bytes);
    const double t_in = now_ms();
    const int32_t rc = comm_allgather_live(e, send, recv, bytes);
    if (!rc && g_rec.recording) record_exchange(recv, bytes, t_in);
    return rc;
}
// The deadline of an exchange (ripp_config.comm_timeout_ms / RIPP_COMM_TIMEOUT_MS, default 60 s).  Status-carrying messages end all ranks together when a
// rank FAILS; a rank that DIES (SIGSEGV, the OOM killer, a GPU fault) never sends its block, and a bare hipStreamSynchronize behind ncclAllGather would hold
// the survivors until somebody kills the job.  The stream is polled instead; on expiry the call returns RIPP_ERR_DEVICE with the exchange's number and the
// communicator is marked broken (the collective is still queued: nothing more can be issued on it, ripp_comm_destroy aborts it).  The CALLER's remedy is a
// non-zero exit or a fresh process -- never a re-exec of this one.  A callback transport keeps its own deadline (the host's process-group timeout); its
// failure is reported the same way.
int32_t comm_allgather_live(Engine* e, const void* send, void* recv, size_t bytes) {
    const uint64_t k = g_comm.n_ex++;
    auto who = [&]() { return "all-gather " + std::to_string(k) + " (" + std::to_string(bytes) + " B per rank), rank " + std::to_string(g_comm.rank) + " of " + std::to_string(g_comm.world); };
    if (g_comm.broken) { set_err(who() + ": the communicator is broken (an earlier exchange ran into its deadline)"); return RIPP_ERR_DEVICE; }
    if (g_comm.cb) {
        const int32_t rc = g_comm.cb(g_comm.cb_user, send, recv, bytes);
        if (rc) { set_err(who() + ": the host's all-gather callback failed (a peer has left the process group, or its deadline passed)"); g_comm.broken = true; }
        return rc ? RIPP_ERR_DEVICE : RIPP_OK;
    }
    int32_t rc; const size_t total = bytes * (size_t)g_comm.world;
    if (!g_comm.st) HIPCHK(hipStreamCreateWithFlags(&g_comm.st, hipStreamNonBlocking));
    if ((rc = g_comm.send.reserve(bytes)) || (rc = g_comm.recv.reserve(total)) || (rc = g_comm.hsend.reserve(bytes)) || (rc = g_comm.hrecv.reserve(total))) return rc;
    std::memcpy(g_comm.hsend.p, send, bytes);
    HIPCHK(hipMemcpyAsync(g_comm.send.p, g_comm.hsend.p, bytes, hipMemcpyHostToDevice, g_comm.st));
    NCCLCHK(g_comm.pAllGather(g_comm.send.p, g_comm.recv.p, bytes, ncclUint8, g_comm.nccl, g_comm.st));
    HIPCHK(hipMemcpyAsync(g_comm.hrecv.p, g_comm.recv.p, total, hipMemcpyDeviceToHost, g_comm.st));
    const double t0 = now_ms(), limit = (double)(e && e->cfg.pub.comm_timeout_ms ? e->cfg.pub.comm_timeout_ms : 60000);
    for (uint32_t spins = 0;; ++spins) {
        const hipError_t q = hipStreamQuery(g_comm.st);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) { set_err(who() + ": " + hipGetErrorString(q)); g_comm.broken = true; return RIPP_ERR_DEVICE; }
        const double waited = now_ms() - t0;
        if (waited > limit) {
            char buf[64]; std::snprintf(buf, sizeof buf, "%.0f", waited);
            set_err(who() + ": no completion after " + buf + " ms -- a peer has died or never entered the exchange; the communicator is unusable");
            g_comm.broken = true; return RIPP_ERR_DEVICE;
        }
        if (spins < 4096) cpu_relax(); else if (waited < 5.0) std::this_thread::yield(); else std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    std::memcpy(recv, g_comm.hrecv.p, total);
    return RIPP_OK;
}
// Self-test of a fresh communicator: one all-gather of (magic, rank, world, ABI version, build fingerprint) checked on EVERY rank -- a mis-wired bring-up
// (two processes with the same rank, ranks of different worlds on one id, two builds of the library in one job) becomes an error string at
// ripp_comm_init instead of a wrong or hanging first proof.
struct CommHello { uint32_t magic, rank, world, abi; uint64_t build; uint64_t pad; };
uint64_t comm_build_fingerprint() {
    const char* s = RIPP_BUILD_STAMP; uint64_t h = 1469598103934665603ull;
    for (; *s; ++s) h = (h ^ (uint8_t)*s) * 1099511628211ull;
    return h ^ (uint64_t)sizeof(ripp_stats) ^ ((uint64_t)sizeof(ripp_config) << 16);
}
int32_t comm_selftest(Engine* e) {
    if (!g_comm.active || g_comm.replay) return RIPP_OK;
    const CommHello mine{0x52495050u, (uint32_t)g_comm.rank, (uint32_t)g_comm.world, (uint32_t)RIPP_ABI_VERSION, comm_build_fingerprint(), 0};
    std::vector<CommHello> all((size_t)g_comm.world);
    if (g_comm.world == 1) all[0] = mine;
    else { const int32_t rc = comm_allgather_live(e, &mine, all.data(), sizeof mine); if (rc) return rc; }
    for (int r = 0; r < g_comm.world; ++r) {
        const CommHello& h = all[(size_t)r];
        std::string bad;
        if (h.magic != mine.magic) bad = "its block is not a greeting of this library";
        else if (h.rank != (uint32_t)r) bad = "it introduced itself as rank " + std::to_string(h.rank);
        else if (h.world != mine.world) bad = "its world size is " + std::to_string(h.world);
        else if (h.abi != mine.abi) bad = "its ABI version is " + std::to_string(h.abi) + ", this rank's " + std::to_string(mine.abi);
        else if (h.build != mine.build) bad = "it runs another build of libripp_hip";
        if (!bad.empty()) { set_err("communicator self-test on rank " + std::to_string(g_comm.rank) + " of " + std::to_string(g_comm.world) + ": slot " + std::to_string(r) + " of the all-gather is wrong: " + bad); return RIPP_ERR_ARG; }
    }
    return RIPP_OK;
}
void comm_reset() {      // back to "no communicator": every field a later call could act on
    if (g_comm.nccl) {       // a broken communicator still has a collective queued: abort it (ncclCommDestroy would wait for it)
        if (g_comm.broken && g_comm.pCommAbort) (void)g_comm.pCommAbort(g_comm.nccl);
        else if (!g_comm.broken && g_comm.pCommDestroy) (void)g_comm.pCommDestroy(g_comm.nccl);
    }
    g_comm.nccl = nullptr; g_comm.n_ex = 0; g_comm.broken = false; g_comm.active = false; g_comm.cb = nullptr; g_comm.cb_user = nullptr; g_comm.rank = 0; g_comm.world = 1;
    g_comm.replay = false; g_rec = Recording();
}
}  // namespace
}  // extern "C++"

API int32_t ripp_comm_unique_id(uint8_t id[128]) {
    if (!id) return RIPP_ERR_ARG;
    LOCK; int32_t rc = rccl_load(); if (rc) return rc;
    ncclUniqueId u; NCCLCHK(g_comm.pGetUniqueId(&u));
    static_assert(sizeof u == 128, "ncclUniqueId"); std::memcpy(id, &u, 128); return RIPP_OK;
}
API int32_t ripp_comm_init(const uint8_t id[128], int32_t rank, int32_t world) {
    if (!id || world < 1 || rank < 0 || rank >= world) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    comm_reset();                                  // a failed bring-up below must not leave the previous communicator's fields behind
    int32_t rc = rccl_load(); if (rc) return rc;
    ncclUniqueId u; std::memcpy(&u, id, 128);
    NCCLCHK(g_comm.pCommInitRank(&g_comm.nccl, world, u, rank));
    g_comm.rank = rank; g_comm.world = world; g_comm.active = true;
    if ((rc = comm_selftest(e))) { comm_reset(); return rc; }
    return RIPP_OK;
}
API int32_t ripp_comm_init_callback(int32_t rank, int32_t world, ripp_allgather_fn allgather, void* user) {
    if (!allgather || world < 1 || rank < 0 || rank >= world) return RIPP_ERR_ARG;
    LOCK;
    comm_reset();
    g_comm.rank = rank; g_comm.world = world; g_comm.cb = allgather; g_comm.cb_user = user; g_comm.active = true;
    { const int32_t rc = comm_selftest(g_engine); if (rc) { comm_reset(); return rc; } }      // (the callback transport needs no device: g_engine may be null)
    return RIPP_OK;
}
// ---- recorded peers: see the comment at `struct Recording` above ----
// file: "RIPPREC1", u32 world, u32 exchanges, then per exchange u32 bytes, u32 0, f64 gap_ms[world] (NaN = not measured), u8 blocks[world][bytes]
API int32_t ripp_comm_record(int32_t on) {
    LOCK;
    if (!g_comm.active || g_comm.replay) { set_err("ripp_comm_record: no live communicator"); return RIPP_ERR_ARG; }
    g_rec.recording = on != 0; g_rec.marked = false;
    if (on) { g_rec.ex.clear(); g_rec.world = g_comm.world; g_rec.t_prev = now_ms(); }
    return RIPP_OK;
}
API int32_t ripp_comm_recording_save(const char* path) {
    if (!path) return RIPP_ERR_ARG;
    LOCK;
    if (g_rec.ex.empty()) { set_err("ripp_comm_recording_save: nothing recorded"); return RIPP_ERR_ARG; }
    FILE* f = std::fopen(path, "wb");
    if (!f) { set_err(std::string("cannot write ") + path); return RIPP_ERR_ARG; }
    const uint32_t hdr[2] = {(uint32_t)g_rec.world, (uint32_t)g_rec.ex.size()};
    bool ok = std::fwrite("RIPPREC1", 1, 8, f) == 8 && std::fwrite(hdr, 4, 2, f) == 2;
    for (const Recording::Ex& x : g_rec.ex) {
        const uint32_t h[2] = {x.bytes, 0};
        ok = ok && std::fwrite(h, 4, 2, f) == 2 && std::fwrite(x.gap.data(), 8, x.gap.size(), f) == x.gap.size() && std::fwrite(x.data.data(), 1, x.data.size(), f) == x.data.size();
    }
    ok = (std::fclose(f) == 0) && ok;
    if (!ok) { set_err(std::string("short write to ") + path); return RIPP_ERR_ARG; }
    return RIPP_OK;
}
API int32_t ripp_comm_init_replay(int32_t rank, int32_t world, const char* path, double latency_us) {
    if (!path || world < 2 || rank < 0 || rank >= world || !(latency_us >= 0)) return RIPP_ERR_ARG;
    LOCK;
    comm_reset();
    FILE* f = std::fopen(path, "rb");
    if (!f) { set_err(std::string("cannot read ") + path); return RIPP_ERR_ARG; }
    char magic[8]; uint32_t hdr[2] = {0, 0};
    bool ok = std::fread(magic, 1, 8, f) == 8 && !std::memcmp(magic, "RIPPREC1", 8) && std::fread(hdr, 4, 2, f) == 2 && hdr[0] == (uint32_t)world && hdr[1] > 0 && hdr[1] < (1u << 20);
    std::vector<Recording::Ex> ex(ok ? hdr[1] : 0);
    for (Recording::Ex& x : ex) {
        uint32_t h[2];
        ok = ok && std::fread(h, 4, 2, f) == 2 && h[0] > 0 && h[0] <= (1u << 24);
        if (!ok) break;
        x.bytes = h[0]; x.gap.resize((size_t)world); x.data.resize((size_t)world * h[0]);
        ok = std::fread(x.gap.data(), 8, x.gap.size(), f) == x.gap.size() && std::fread(x.data.data(), 1, x.data.size(), f) == x.data.size();
    }
    std::fclose(f);
    if (!ok) { set_err(std::string(path) + ": not a recording of a " + std::to_string(world) + "-rank proof"); return RIPP_ERR_ARG; }
    g_rec.ex = std::move(ex); g_rec.world = world; g_rec.latency_ms = latency_us * 1e-3;
    g_comm.rank = rank; g_comm.world = world; g_comm.replay = true; g_comm.active = true;
    return RIPP_OK;
}
// what the replay has done so far: exchanges served, how many of this rank's own blocks differed from the recorded ones (timing fields of the
// plan message do; a GT value must not -- the proof comparison catches that), time spent inside the exchanges (waiting for the modelled peers)
API int32_t ripp_comm_replay_info(uint64_t* served, uint64_t* own_differs, double* waited_ms) {
    LOCK;
    if (served) *served = g_rec.served; if (own_differs) *own_differs = g_rec.own_differs; if (waited_ms) *waited_ms = g_rec.waited_ms;
    return RIPP_OK;
}
extern "C++" {
namespace {
bool ex_same_meaning(uint8_t kind, const uint8_t* a, const uint8_t* b, size_t bytes) {
    if (!std::memcmp(a, b, bytes)) return true;
    switch (kind) {
    case EX_PLAN: return bytes >= 16 && !std::memcmp(a, b, 16);                 // n_local, world, rank; what follows are the plan and clock readings of that run
    case EX_GT: {
        if (bytes % sizeof(Fp12)) return false;
        for (size_t k = 0; k < bytes / sizeof(Fp12); ++k) {
            Fp12 x, y; std::memcpy(&x, a + k * sizeof(Fp12), sizeof x); std::memcpy(&y, b + k * sizeof(Fp12), sizeof y);
            if (!std::memcmp(&x, &y, sizeof x)) continue;
            const Fp12 fx = final_exponentiation(x), fy = final_exponentiation(y);
            if (std::memcmp(&fx, &fy, sizeof fx)) return false;
        }
        return true; }
    case EX_G1J: case EX_G2J: {
        const size_t es = kind == EX_G1J ? sizeof(G1J) : sizeof(G2J);
        if (bytes % es) return false;
        for (size_t k = 0; k < bytes / es; ++k) {
            if (kind == EX_G1J) { G1J x, y; std::memcpy(&x, a + k * es, es); std::memcpy(&y, b + k * es, es); const G1A ax = to_affine(x), ay = to_affine(y); if (std::memcmp(&ax, &ay, sizeof ax)) return false; }
            else { G2J x, y; std::memcpy(&x, a + k * es, es); std::memcpy(&y, b + k * es, es); const G2A ax = to_affine(x), ay = to_affine(y); if (std::memcmp(&ax, &ay, sizeof ax)) return false; }
        }
        return true; }
    default: return false;
    }
}
}
}
// The replay's verdict on the live rank's own blocks (run AFTER the timed proofs): every block whose bytes differed from the recording is compared by kind
// (see ExKind).  differing = such blocks; mismatches = those that also MEAN something else -- a protocol divergence; non-zero => RIPP_ERR_ARG and the first one named.
API int32_t ripp_comm_replay_check(uint64_t* differing, uint64_t* mismatches) {
    LOCK;
    for (const Recording::Differing& d : g_rec.differing) {
        bool ok;
        if (!d.d.mux) ok = ex_same_meaning(d.d.k0, d.live.data(), d.rec.data(), d.live.size());
        else ok = d.live.size() == 8u + d.d.b0 + d.d.b1 && !std::memcmp(d.live.data(), d.rec.data(), 8)
                  && (!d.d.b0 || ex_same_meaning(d.d.k0, d.live.data() + 8, d.rec.data() + 8, d.d.b0)) && (!d.d.b1 || ex_same_meaning(d.d.k1, d.live.data() + 8 + d.d.b0, d.rec.data() + 8 + d.d.b0, d.d.b1));
        if (!ok) { if (!g_rec.mismatches) g_rec.first_mismatch = "exchange " + std::to_string(d.ex) + " (" + std::to_string(d.live.size()) + " B, kind " + std::to_string(d.d.k0) + (d.d.mux ? "/" + std::to_string(d.d.k1) + ", paired" : "") + ")"; ++g_rec.mismatches; }
    }
    if (differing) *differing = g_rec.own_differs; if (mismatches) *mismatches = g_rec.mismatches;
    g_rec.differing.clear();
    if (g_rec.mismatches) { set_err("replay: this rank's own block differs IN MEANING from the recorded one at " + g_rec.first_mismatch + ": the live run has left the recorded protocol"); return RIPP_ERR_ARG; }
    return RIPP_OK;
}
API void ripp_comm_destroy(void) {
    LOCK;
    if (g_comm.st && !g_comm.broken) (void)hipStreamSynchronize(g_comm.st);
    comm_reset();
    g_comm.send.release(); g_comm.recv.release(); g_comm.hsend.release(); g_comm.hrecv.release();
    if (g_comm.st) { (void)hipStreamDestroy(g_comm.st); g_comm.st = nullptr; }
}
API int32_t ripp_comm_rank(void) { return g_comm.active ? g_comm.rank : 0; }
API int32_t ripp_comm_world(void) { return g_comm.active ? g_comm.world : 1; }
API int32_t ripp_comm_allgather(const void* send, void* recv, size_t bytes) {
    if (!send || !recv) return RIPP_ERR_ARG;
    LOCK; ENGINE; return comm_allgather(e, send, recv, bytes);
}

