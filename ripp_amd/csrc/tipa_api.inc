// Included by engine.hip inside its `extern "C"` block (after the Engine, the SIPP job internals and the basic C-ABI entry points).
// The callers directly above the hot path: GIPA / TIPA / TIPAWithSSM provers, aggregate_proofs, and the verifiers.
// ---- GIPA / TIPP prover (ip_proofs/src/gipa.rs:181-312) ------------------------------------------------------------------
// The four vectors are kept AFFINE on the device between rounds (each commitment of the reference re-normalises its
// projective inputs anyway, inner_products/src/lib.rs:80-81; group elements are identical), the six commitments of a
// round share ONE line launch, and the folds reuse the NAF / GLS kernels: G1 vectors take the full-width c, G2 vectors
// the 128-bit c_inv -- exactly the reference's choice (gipa.rs:252-256).
extern "C++" {
// second base of a fold in the VM regime (vm_fold2.hpp): 2^64 hi (G1) / 2^32 hi (G2) in projective form, prepared while the host
// finishes the round's GT values; `ready` is consumed by the next fold_dev on the same vector
struct FoldPre { DevBuf pow_h, parts; bool ready = false; void release() { pow_h.release(); parts.release(); } };
// The per-call vector sets (TippVecs / SsmVecs / MexpVecs / ScalVecs) hand their device buffers to one of these when they go out of scope and the next set adopts them:
// a call of aggregate_proofs at n = 2^14 made ~35 hipMalloc / hipFree pairs, and a hipFree of >= 1 MB costs 60-120 us on this runtime (2-4 ms per call).
// Freed by ripp_release_scratch / ripp_shutdown (vec_caches_release).  All users hold the engine lock.
struct VecBufCache { std::vector<DevBuf> bufs; bool full = false;
    void adopt(const std::vector<DevBuf*>& l) { if (!full || bufs.size() != l.size()) return; size_t i = 0; for (DevBuf* b : l) std::swap(*b, bufs[i++]); full = false; }
    // park() synchronises the device first: a prover that returns early on an error may leave kernels of this call in flight on the engine's (or
    // the auxiliary engine's) streams, and the next call adopts the same buffers, possibly on other streams.  ~10 us on an idle device, once per call.
    void park(const std::vector<DevBuf*>& l) { (void)hipDeviceSynchronize(); if (full) { for (DevBuf* b : l) b->release(); return; } bufs.resize(l.size()); size_t i = 0; for (DevBuf* b : l) { bufs[i].release(); std::swap(*b, bufs[i++]); } full = true; }
    void release() { for (DevBuf& b : bufs) b.release(); full = false; } };
static VecBufCache g_tipp_cache, g_ssm_cache, g_mexp_cache, g_scal_cache;      // (g_mexp_cache: the vector set of gipa_mexp_api.inc and tipa_mexp_api.inc, g_scal_cache: that of tipa_scalar_api.inc)
// A vector set's hold on its buffers: adopts the cache's parked buffers when the set is built and parks them when it goes.  cache == nullptr: the set of one
// in-process rank (its own device: never into the process-wide parking place), synchronised and released instead.  Declare it as the LAST member of the set:
// members die in reverse order, so the lease parks while the DevBufs are still alive (as a base class it would run after they are gone).
struct VecLease { VecBufCache* cache; std::vector<DevBuf*> bufs;
    VecLease(VecBufCache* c, std::initializer_list<DevBuf*> l) : cache(c), bufs(l) { if (cache) cache->adopt(bufs); }
    ~VecLease() { if (cache) cache->park(bufs); else { (void)hipDeviceSynchronize(); for (DevBuf* b : bufs) b->release(); } }
    VecLease(const VecLease&) = delete; VecLease& operator=(const VecLease&) = delete; };
static FoldPre g_tpc_pre;                  // second fold base of the first-tier key folds (tpc_api.inc)
static void vec_caches_release() { g_tipp_cache.release(); g_ssm_cache.release(); g_mexp_cache.release(); g_scal_cache.release(); g_tpc_pre.release(); }
template <class F> static int32_t fold_precompute(Engine* e, hipStream_t st, const Affine<F>* hi, size_t half, FoldPre& fp) {
    fp.ready = false;
    if (half == 0 || half > e->cfg.pub.vm_fold_max || e->cfg.pub.no_vm || e->cfg.pub.no_precompute) return RIPP_OK;
    constexpr bool g1 = std::is_same<F, Fp>::value;
    int32_t rc; if ((rc = fp.pow_h.reserve(half * sizeof(Jac<F>))) || (rc = fp.parts.reserve((g1 ? 4 : 8) * half * sizeof(Jac<F>)))) return rc;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_vm_pow2<F>), dim3(nblk(half, 4 * VM_EPW)), dim3(256), 4 * VM_EPW * VmCurve<F>::SLOTS * sizeof(VmSlot), st, hi, (uint32_t)half, g1 ? 64 : 32, fp.pow_h.as<Jac<F>>());
    HIPCHK(hipGetLastError());
    fp.ready = true; return RIPP_OK;
}
// Batched small-round forms: the second bases resp. the folds of up to three vectors of one group in ONE launch sequence on one stream
// (vm_fold2.hpp: grid.z / grid.y = vector), ending in affine points.
template <class F> struct FoldReq { const Affine<F>* hi; const Affine<F>* lo; Affine<F>* out; Fr s; FoldPre* fp; };
static bool fold_batching(const Engine* e, size_t half) { return half != 0 && half <= e->cfg.pub.vm_fold_max && !e->cfg.pub.no_vm && !e->cfg.pub.no_precompute; }
template <class F> static int32_t fold_precompute_batch(Engine* e, hipStream_t st, FoldReq<F>* req, int cnt, size_t half) {
    constexpr bool g1 = std::is_same<F, Fp>::value;
    Pow2Batch<F> pb{};
    for (int v = 0; v < cnt; ++v) {
        FoldPre& fp = *req[v].fp; fp.ready = false;
        int32_t rc; if ((rc = fp.pow_h.reserve(half * sizeof(Jac<F>))) || (rc = fp.parts.reserve((g1 ? 4 : 8) * half * sizeof(Jac<F>)))) return rc;
        pb.in[v] = req[v].hi; pb.out_h[v] = fp.pow_h.as<Jac<F>>();
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_vm_pow2_b<F>), dim3(nblk(half, 4 * VM_EPW), cnt), dim3(256), 4 * VM_EPW * VmCurve<F>::SLOTS * sizeof(VmSlot), st, pb, (uint32_t)half, g1 ? 64 : 32);
    HIPCHK(hipGetLastError());
    for (int v = 0; v < cnt; ++v) req[v].fp->ready = true;
    return RIPP_OK;
}
template <class F> static int32_t fold_batch_dev(Engine* e, hipStream_t st, FoldReq<F>* req, int cnt, size_t half) {
    constexpr bool g1 = std::is_same<F, Fp>::value;
    constexpr int rows = g1 ? 4 : 8;
    FoldBatch<F> fb{};
    for (int v = 0; v < cnt; ++v) {
        FoldPre& fp = *req[v].fp; fp.ready = false;
        fb.s[v] = {req[v].hi, fp.pow_h.as<Jac<F>>(), req[v].lo, fp.parts.as<Jac<F>>(), req[v].out};
        if constexpr (g1) fb.dg[v] = split_digits_g1_glv(req[v].s); else fb.dg[v] = split_digits_g2(req[v].s);
    }
    const size_t lds = 4 * VM_EPW * VmCurve<F>::SLOTS * sizeof(VmSlot);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_vm_fold_split2_b<F>), dim3(nblk(half, 4 * VM_EPW), rows, cnt), dim3(256), lds, st, fb, (uint32_t)half, rows / 2);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_vm_combine_aff_b<F>), dim3(nblk(half, 4 * VM_EPW), cnt), dim3(256), lds, st, fb, rows, (uint32_t)half);
    HIPCHK(hipGetLastError());
    return RIPP_OK;
}
template <class F> static int32_t fold_dev(Engine* e, hipStream_t st, const Affine<F>* hi, const Affine<F>* lo, size_t half, const Fr& s, DevBuf& jac, DevBuf& qt, Affine<F>* out, FoldPre* fp = nullptr);
template <> int32_t fold_dev<Fp>(Engine* e, hipStream_t st, const G1A* hi, const G1A* lo, size_t half, const Fr& s, DevBuf& jac, DevBuf&, G1A* out, FoldPre* fp) {
    int32_t rc; if ((rc = jac.reserve(half * sizeof(G1J)))) return rc;
    if (fp && fp->ready && half <= e->cfg.pub.vm_fold_max) {            // four 64-bit digit strings on four lane groups: 64 doublings on the chain instead of 128
        fp->ready = false;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_vm_fold_split2<Fp>), dim3(nblk(half, 4 * VM_EPW), 4), dim3(256), 4 * VM_EPW * VmCurve<Fp>::SLOTS * sizeof(VmSlot), st, hi, fp->pow_h.as<G1J>(), (uint32_t)half, split_digits_g1_glv(s), 2, fp->parts.as<G1J>());
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_vm_combine<Fp>), dim3(nblk(half, 4 * VM_EPW)), dim3(256), 4 * VM_EPW * VmCurve<Fp>::SLOTS * sizeof(VmSlot), st, fp->parts.as<G1J>(), 4, lo, (uint32_t)half, jac.as<G1J>());
        HIPCHK(hipGetLastError());
        return e->normalize_dev<Fp>(jac.as<G1J>(), half, out, st);
    }
    if (fp) fp->ready = false;
    // GIPA folds G1 vectors with the full-width challenge c: split it through the GLV endomorphism (128 doublings instead of 255)
    if (half <= e->cfg.pub.vm_fold_max && !e->cfg.pub.no_vm)     // latency form (complete additions, nothing to flag)
        hipLaunchKernelGGL(k_vm_fold_g1_glv, dim3(nblk(half, 4 * VM_EPW)), dim3(256), 4 * VM_EPW * VM_G1_SLOTS * sizeof(VmSlot), st, hi, lo, (uint32_t)half, glv_digits(s), jac.as<G1J>());
    else if (!e->cfg.pub.no_fq)                          // throughput / mid-size rounds: the carry-free twin (fq_curve.hpp)
        hipLaunchKernelGGL(k_fold_g1_glv_q, dim3(nblk(half, 256)), dim3(256), 0, st, hi, lo, (uint32_t)half, glv_digits(s), jac.as<G1J>());
    else
        hipLaunchKernelGGL(k_fold_g1_glv, dim3(nblk(half, 256)), dim3(256), 0, st, hi, lo, (uint32_t)half, glv_digits(s), jac.as<G1J>());
    HIPCHK(hipGetLastError());
    return e->normalize_dev<Fp>(jac.as<G1J>(), half, out, st);
}
template <> int32_t fold_dev<Fp2>(Engine* e, hipStream_t st, const G2A* hi, const G2A* lo, size_t half, const Fr& s, DevBuf& jac, DevBuf& qt, G2A* out, FoldPre* fp) {
    int32_t rc; if ((rc = jac.reserve(half * sizeof(G2J)))) return rc;
    if (fp && fp->ready && half <= e->cfg.pub.vm_fold_max) {            // eight 32-bit digit strings on eight lane groups
        fp->ready = false;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_vm_fold_split2<Fp2>), dim3(nblk(half, 4 * VM_EPW), 8), dim3(256), 4 * VM_EPW * VmCurve<Fp2>::SLOTS * sizeof(VmSlot), st, hi, fp->pow_h.as<G2J>(), (uint32_t)half, split_digits_g2(s), 4, fp->parts.as<G2J>());
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_vm_combine<Fp2>), dim3(nblk(half, 4 * VM_EPW)), dim3(256), 4 * VM_EPW * VmCurve<Fp2>::SLOTS * sizeof(VmSlot), st, fp->parts.as<G2J>(), 8, lo, (uint32_t)half, jac.as<G2J>());
        HIPCHK(hipGetLastError());
        return e->normalize_dev<Fp2>(jac.as<G2J>(), half, out, st);
    }
    if (fp) fp->ready = false;
    const size_t qstride = (half + 63) & ~(size_t)63;
    const size_t qt_bytes = std::max<size_t>(4 * G2A_CHUNKS * qstride * sizeof(uint4), 4 * half * sizeof(G2J));
    if ((rc = qt.reserve(qt_bytes + 4 * half + 16)) || (rc = e->vm_flag.reserve(sizeof(uint32_t)))) return rc;          // (vm_flag: a vestigial argument of k_vm_fold_g2_split; + one flag byte per lane of the carry-free GLS fold, behind the parts: this call's own scratch, the two G2 folds of a round may run side by side)
    if (half <= e->cfg.pub.vm_fold_max && !e->cfg.pub.no_vm) {
        hipLaunchKernelGGL(k_vm_fold_g2_split, dim3(nblk(half, 4 * VM_EPW), 4), dim3(256), 4 * VM_EPW * VM_G2_SLOTS * sizeof(VmSlot), st, hi, (uint32_t)half, gls_digits(s), qt.as<G2J>(), e->vm_flag.as<uint32_t>());
        hipLaunchKernelGGL(k_vm_combine_g2, dim3(nblk(half, 4 * VM_EPW)), dim3(256), 4 * VM_EPW * VM_G2_SLOTS * sizeof(VmSlot), st, qt.as<G2J>(), lo, (uint32_t)half, jac.as<G2J>());
    } else if (half <= e->cfg.pub.gls_split_max) {
        if (!e->cfg.pub.no_fq) {
            uint8_t* flags = qt.as<uint8_t>() + qt_bytes;
            hipLaunchKernelGGL(k_fold_g2_gls_split_q, dim3(nblk(half, 64), 4), dim3(64), 0, st, hi, (uint32_t)half, gls_digits(s), qt.as<G2J>(), flags);
#if !defined(RIPP_INLINE_FALLBACK)
            hipLaunchKernelGGL(k_fold_g2_gls_split_fix, dim3(FIX_GRID), dim3(64), 0, st, hi, (uint32_t)half, gls_digits(s), qt.as<G2J>(), flags);
#endif
        } else
        hipLaunchKernelGGL(k_fold_g2_gls_split, dim3(nblk(half, 64), 4), dim3(64), 0, st, hi, (uint32_t)half, gls_digits(s), qt.as<G2J>());
        hipLaunchKernelGGL(k_fold_g2_combine, dim3(nblk(half, 64)), dim3(64), 0, st, qt.as<G2J>(), lo, (uint32_t)half, jac.as<G2J>());
    } else if (fold_g2_table_pays(e, half)) {                    // two G2 folds of a round share the stream, hence the table buffers
        if ((rc = fold_g2_table(e, st, hi, lo, half, s, jac))) return rc;
    } else {
        hipLaunchKernelGGL(k_fold_g2_gls, dim3(nblk(half, 64)), dim3(64), 0, st, hi, lo, (uint32_t)half, gls_digits(s), qt.as<uint4>(), qstride, jac.as<G2J>());
    }
    HIPCHK(hipGetLastError());
    return e->normalize_dev<Fp2>(jac.as<G2J>(), half, out, st);
}
}  // extern "C++"

extern "C++" { static Fp12 gt_pow_host(const Fp12& x, const Fr& k); }      // defined with the verifiers below

extern "C++" {
// k-th power of an element of GT PROPER (order r).  The Frobenius acts there as the power p = x (mod r), so with u = |x|
//     z^(u^j) = conj^j(frobenius^j(z))          (conj = inverse in the cyclotomic subgroup; x < 0 on BLS12-381 -- on BLS12-377 x = u > 0 and no conjugation),
// and the exponent is written in base u like the scalars of the G2 folds: 64 cyclotomic squarings + ~85 products instead of 255 + ~85.
// Only for values this library produced itself (outputs of a final exponentiation): proof-supplied elements are checked to be
// cyclotomic, not to have order r, so the verifiers keep the plain form (gt_pow_host).
// `strings`: bit j set = digit string j takes part; the product over a partition of the four strings is the whole power, so the strings of one
// exponentiation can run on different host threads (64 squarings + ~21 products per string instead of 64 + ~85 on one thread).
static Fp12 gt_pow_gls_strings(const Fp12& z, const GlsDigits& g, unsigned strings) {
    Fp12 b[4], bi[4];
    b[0] = z;
    for (int j = 1; j < 4; ++j) if ((strings >> j) & 1u) { b[j] = frobenius(z, j); if (BLS_X_NEG && (j & 1)) b[j] = conj(b[j]); }      // z^(x^j) = frobenius^j(z); u = -x on BLS12-381
    for (int j = 0; j < 4; ++j) if ((strings >> j) & 1u) bi[j] = conj(b[j]);
    Fp12 acc = Fp12::one(); bool st = false;
    for (int pos = g.len - 1; pos >= 0; --pos) {
        if (st) acc = cyclotomic_sqr(acc);
        for (int j = 0; j < 4; ++j) {
            if (!((strings >> j) & 1u)) continue;
            const int d = g.d[j][pos];
            if (d != 0) { const Fp12& m = d > 0 ? b[j] : bi[j]; acc = st ? mul(acc, m) : m; st = true; }
        }
    }
    return acc;
}
static Fp12 gt_pow_gls(const Fp12& z, const Fr& k) { return gt_pow_gls_strings(z, gls_digits(k), 15u); }
}  // extern "C++"

// device-resident GIPA/TIPP state: the four vectors (affine) + ping-pong partners + fold scratch
struct TippVecs {
    DevBuf A, A2, KB, KB2, B, B2, KA, KA2, jac1, jac1b, jac2, jac2b, qt2;
    DevBuf AU, AU2, jac1u;                 // implicit-shift form (aggregate_proofs): the UNSCALED left vector beside the scaled one
    FoldPre pA, pKB, pB, pKA, pAU;         // second fold bases of the small rounds
    VecLease lease;                        // (last member)
    explicit TippVecs(bool use_cache = true)      // false: the buffers of one in-process rank
        : lease(use_cache ? &g_tipp_cache : nullptr, {&A, &A2, &KB, &KB2, &B, &B2, &KA, &KA2, &jac1, &jac1b, &jac2, &jac2b, &qt2, &AU, &AU2, &jac1u, &pA.pow_h, &pA.parts, &pKB.pow_h, &pKB.parts,
                                                       &pB.pow_h, &pB.parts, &pKA.pow_h, &pKA.parts, &pAU.pow_h, &pAU.parts}) {}
    int32_t reserve(size_t n) {
        int32_t rc;
        for (DevBuf* b : {&A, &A2, &KB, &KB2}) if ((rc = b->reserve(n * sizeof(G1A)))) return rc;
        for (DevBuf* b : {&B, &B2, &KA, &KA2}) if ((rc = b->reserve(n * sizeof(G2A)))) return rc;
        if ((rc = jac1.reserve(n * sizeof(G1J))) || (rc = jac2.reserve(n * sizeof(G2J)))) return rc;
        return RIPP_OK;
    }
};

extern "C++" {
// one round's folds: the four side streams wait for the engine's stream, `launch` enqueues the folds on whichever of the five it likes, the engine's stream
// waits for all of them and is synchronised.  (The VM folds use the complete addition law: there is no exceptional case to detect and redo.)
template <class Launch> static int32_t fork_join_folds(Engine* e, Launch&& launch) {
    int32_t rc;
    HIPCHK(hipEventRecord(e->ev_fork, e->stream));
    for (hipStream_t st : {e->stream2, e->stream3, e->stream4, e->stream5}) HIPCHK(hipStreamWaitEvent(st, e->ev_fork, 0));
    if ((rc = launch())) return rc;
    HIPCHK(hipEventRecord(e->ev_join, e->stream2)); HIPCHK(hipEventRecord(e->ev_join3, e->stream3)); HIPCHK(hipEventRecord(e->ev_join4, e->stream4)); HIPCHK(hipEventRecord(e->ev_join5, e->stream5));
    for (hipEvent_t ev : {e->ev_join, e->ev_join3, e->ev_join4, e->ev_join5}) HIPCHK(hipStreamWaitEvent(e->stream, ev, 0));
    return e->sync();
}
}  // extern "C++"

// ---- sharding of the GIPA-family provers (SURVEY.md section 8e) ------------------------------------------------------------------------
// One process per GPU, every vector partitioned by index residue (global element i = j * world + rank is local element j of rank
// i mod world), so the two halves of a round are co-resident and every fold is local.  Per round a rank contributes ITS Miller values
// (before the final exponentiation) resp. ITS partial MSM sums; they are all-gathered (576 B / 144 B each) and multiplied / added --
// RCCL has no reduction over Fq12 products or curve points.  When every rank is down to one element the `world` survivors of each
// vector are gathered and the last log2(world) rounds run replicated.  world == 1 is the unsharded prover, bit for bit.
extern "C++" {
struct ShardCtx {
    int rank = 0, world = 1;
    static ShardCtx from_comm() { ShardCtx s; if (t_lcomm) { s.rank = t_lrank; s.world = t_lcomm->world; return s; } s.rank = g_comm.active ? g_comm.rank : 0; s.world = g_comm.active ? g_comm.world : 1; return s; }
};
// vals[count] <- element-wise product over ranks (Miller values / GT partials)
static int32_t shard_mul_gt(Engine* e, const ShardCtx& sc, Fp12* vals, int count) {
    if (sc.world == 1) return RIPP_OK;
    std::vector<Fp12> all((size_t)sc.world * count);
    t_ex_kind = EX_GT;
    int32_t rc = comm_allgather(e, vals, all.data(), (size_t)count * sizeof(Fp12)); if (rc) return rc;
    for (int k = 0; k < count; ++k) { Fp12 acc = all[k]; for (int w = 1; w < sc.world; ++w) acc = mul(acc, all[(size_t)w * count + k]); vals[k] = acc; }
    return RIPP_OK;
}
// pts[count] <- element-wise sum over ranks (partial MSM results)
template <class F> static int32_t shard_add_pts(Engine* e, const ShardCtx& sc, Jac<F>* pts, int count) {
    if (sc.world == 1) return RIPP_OK;
    std::vector<Jac<F>> all((size_t)sc.world * count);
    t_ex_kind = std::is_same<F, Fp>::value ? EX_G1J : EX_G2J;
    int32_t rc = comm_allgather(e, pts, all.data(), (size_t)count * sizeof(Jac<F>)); if (rc) return rc;
    for (int k = 0; k < count; ++k) { Jac<F> acc = all[k]; for (int w = 1; w < sc.world; ++w) acc = add(acc, all[(size_t)w * count + k]); pts[k] = acc; }
    return RIPP_OK;
}
// tail of a sharded vector: every rank holds ONE element in buf; afterwards buf holds the `world` elements in rank (= global) order
template <class T> static int32_t shard_gather_tail(Engine* e, const ShardCtx& sc, DevBuf& buf) {
    T mine; HIPCHK(hipMemcpy(&mine, buf.p, sizeof mine, hipMemcpyDeviceToHost));
    std::vector<T> all((size_t)sc.world);
    int32_t rc = comm_allgather(e, &mine, all.data(), sizeof mine); if (rc) return rc;
    if ((rc = buf.reserve((size_t)sc.world * sizeof(T))) || (rc = e->stage[3].reserve((size_t)sc.world * sizeof(T)))) return rc;
    std::memcpy(e->stage[3].p, all.data(), (size_t)sc.world * sizeof(T));
    if ((rc = e->stage[3].send(buf.p, (size_t)sc.world * sizeof(T), e->stream))) return rc;
    return e->stage[3].wait();
}
// ---- small helpers of every caller below and of poly_commit_api.inc / tpc_api.inc ------------------------------------------------------------------
static bool is_pow2(size_t v) { return v != 0 && !(v & (v - 1)); }
static size_t log2_sz(size_t v) { size_t l = 0; while (((size_t)1 << l) < v) ++l; return l; }
static std::vector<Fr> fr_powers(const Fr& s, size_t n) { std::vector<Fr> p(n); if (n) p[0] = Fr::one(); for (size_t i = 1; i < n; ++i) p[i] = mul(p[i - 1], s); return p; }      // structured_scalar_power
// the sqrt split of a univariate degree (poly_commit/mod.rs:299-306, transparent.rs:221-227): the skew factor is min(skew_cap, sqrt / 2); who / cite: the error text's
static int32_t sqrt_split(size_t degree, size_t skew_cap, const char* who, const char* cite, size_t* x_degree, size_t* y_degree) {
    if (!x_degree || !y_degree || degree >= ((size_t)1 << 62)) return RIPP_ERR_ARG;
    const size_t v = degree + 1;
    size_t lo = 0, hi = (size_t)1 << 31;                                                // floor(sqrt(v)) by bisection, then its ceiling
    while (lo < hi) { const size_t mid = (lo + hi + 1) / 2; if (mid <= v / mid) lo = mid; else hi = mid - 1; }
    const size_t s = lo * lo == v ? lo : lo + 1;
    size_t sq = 1; while (sq < s) sq <<= 1;                                              // next_power_of_two
    const size_t skew = std::min(skew_cap, sq / 2);
    if (skew == 0) { set_err(std::string(who) + ": degree 0 has no split (the reference divides by a zero skew factor, " + cite + ")"); return RIPP_ERR_ARG; }
    *x_degree = sq / skew - 1; *y_degree = sq * skew - 1;
    return RIPP_OK;
}
// the end of a prover call: kernel times, wall time and (with_bytes) the resident device bytes into e->stats, a copy to the caller
static int32_t finish_stats(Engine* e, double t_start, ripp_stats* st, bool with_bytes = true) {
    e->collect_kernel_stats();
    e->stats.total_ms = now_ms() - t_start; if (with_bytes) e->stats.device_bytes = g_dev_bytes.load(std::memory_order_relaxed);
    if (st) *st = e->stats;
    return RIPP_OK;
}
}  // extern "C++"

// GIPA::_prove (gipa.rs:181-312) on vectors already resident (and normalised) in v.A (m_a), v.B (m_b), v.KA (ck_a), v.KB (ck_b).
//
// shift != nullptr -- the implicit-shift form used by aggregate_proofs, where m_a[i] = r^i a_i and ck_a[i] = r^-i ck_i
// (groth16_aggregation.rs:119-131).  The n G2 scalar multiplications r^-i ck_i are never performed: v.KA holds the UNSCALED keys and
// v.AU the unscaled a_i next to the scaled v.A.  By bilinearity e(r^(i+s) a_(i+s), r^-i ck_i) = e(a_(i+s), ck_i)^(r^s), so the two
// LMC commitments of a round are the unscaled products raised to r^(+-split) (two GT exponentiations on host threads), and the
// folds of the unscaled vectors keep the invariant "element i carries the implicit factor r^(+-i)" when they use the scalars
// c r^split and c_inv r^-split.  Index 0 carries r^0, so the final key and every output are the SAME group elements as in the
// explicit computation -- bit-identical results, checked against the oracle's explicit form.
// n = LOCAL length (this rank's shard); sc: the sharding (world == 1: the whole vectors)
static int32_t gipa_tipp_core(Engine* e, TippVecs& v, size_t n, ripp_gt* com_steps, ripp_fr* transcript, G1A& ha, G2A& hb, G2A& hka, G1A& hkb, const Fr* shift = nullptr, ShardCtx sc = ShardCtx()) {
    int32_t rc;
    size_t len = n, round = 0;
    Fr prev_c = Fr::zero();
    std::vector<Fp12> rows(6 * N_LINES);
    std::vector<Fr> rp, rpi;                   // r^(2^k), r^-(2^k), k up to log2 of the GLOBAL length
    if (shift) { rp.push_back(*shift); rpi.push_back(inv(*shift)); for (size_t m = 2; m < n * (size_t)sc.world; m <<= 1) { rp.push_back(mul(rp.back(), rp.back())); rpi.push_back(mul(rpi.back(), rpi.back())); } }
    for (;;) {
        if (len == 1) {
            if (sc.world == 1) break;
            // every rank is down to one element per vector: gather the survivors, finish replicated
            if ((rc = shard_gather_tail<G1A>(e, sc, v.A)) || (rc = shard_gather_tail<G1A>(e, sc, v.KB)) || (rc = shard_gather_tail<G2A>(e, sc, v.B)) || (rc = shard_gather_tail<G2A>(e, sc, v.KA))) return rc;
            if (shift && (rc = shard_gather_tail<G1A>(e, sc, v.AU))) return rc;
            len = (size_t)sc.world; sc.world = 1;
            if ((rc = v.reserve(len)) || (shift && ((rc = v.AU2.reserve(len * sizeof(G1A))) || (rc = v.jac1u.reserve(len * sizeof(G1J)))))) return rc;
            continue;
        }
        const size_t split = len / 2;
        const G1A *A = v.A.as<G1A>(), *KB = v.KB.as<G1A>(); const G2A *B = v.B.as<G2A>(), *KA = v.KA.as<G2A>();
        const G1A* AL = shift ? v.AU.as<G1A>() : A;         // left operand of the two LMC commitments
        const size_t lg_split = log2_sz(split * (size_t)sc.world);      // exponent index of the GLOBAL split
        //            com_1.0 (m_a_1,ck_a_1)  com_1.1 (ck_b_1,m_b_1)  com_1.2 (m_a_1,m_b_1)  com_2.0 (m_a_2,ck_a_2)  com_2.1 (ck_b_2,m_b_2)  com_2.2 (m_a_2,m_b_2)   gipa.rs:209-231
        const G1A* as[6] = {AL + split,            KB + split,            A + split,             AL,                    KB,                    A};
        const G2A* bs[6] = {KA,                    B,                     B,                     KA + split,            B + split,             B + split};
        const double tp = now_ms();
        if ((rc = e->step_products(as, bs, 6, split, rows.data()))) return rc;
        e->stats.miller_products_ms += now_ms() - tp;
        // small rounds: second bases of the four (five) folds on the VM while the host finishes the six commitments -- one batched
        // launch per group (the scalars are filled in once the challenge is known)
        const bool batch = fold_batching(e, split);
        FoldReq<Fp> rq1[3] = {{A + split, A, v.A2.as<G1A>(), Fr::zero(), &v.pA}, {KB + split, KB, v.KB2.as<G1A>(), Fr::zero(), &v.pKB}, {AL + split, AL, v.AU2.as<G1A>(), Fr::zero(), &v.pAU}};
        FoldReq<Fp2> rq2[2] = {{B + split, B, v.B2.as<G2A>(), Fr::zero(), &v.pB}, {KA + split, KA, v.KA2.as<G2A>(), Fr::zero(), &v.pKA}};
        if (batch) {
            if ((rc = fold_precompute_batch<Fp>(e, e->stream2, rq1, shift ? 3 : 2, split)) || (rc = fold_precompute_batch<Fp2>(e, e->stream, rq2, 2, split))) return rc;
        }
        const double th = now_ms();
        Fp12 com[6];
        if (sc.world > 1) {          // this rank's six Miller values -> product over ranks (the f <- f^2 L recurrence is multiplicative)
            std::vector<std::future<Fp12>> fut;
            for (int k = 1; k < 6; ++k) fut.push_back(host_pool().submit([&rows, k]() { return miller_combine(rows.data() + k * N_LINES); }));
            com[0] = miller_combine(rows.data());
            for (int k = 1; k < 6; ++k) com[k] = fut[k - 1].get();
            if ((rc = shard_mul_gt(e, sc, com, 6))) return rc;
        }
        { std::vector<std::future<Fp12>> fut;
          const bool have_ml = sc.world > 1;
          auto one = [&rows, &com, have_ml, shift, &rp, &rpi, lg_split](int k) {
              Fp12 z = final_exponentiation(have_ml ? com[k] : miller_combine(rows.data() + k * N_LINES));
              if (shift && k == 0) z = gt_pow_gls(z, rp[lg_split]);              // (prod e(a_(i+s), ck_i))^(r^s)
              if (shift && k == 3) z = gt_pow_gls(z, rpi[lg_split]);             // (prod e(a_i, ck_(i+s)))^(r^-s)
              return z; };
          for (int k = 1; k < 6; ++k) fut.push_back(host_pool().submit([one, k]() { return one(k); }));
          const Fp12 z0 = one(0);
          Fp12 zs[6]; zs[0] = z0;
          for (int k = 1; k < 6; ++k) zs[k] = fut[k - 1].get();
          for (int k = 0; k < 6; ++k) com[k] = zs[k]; }
        Fr c_inv; const Fr c = fs::gipa_challenge(round ? &prev_c : nullptr, fs::Com{com[0], com[1], com[2]}, fs::Com{com[3], com[4], com[5]}, c_inv);
        const Fr c_u = shift ? mul(c, rp[lg_split]) : c, c_inv_u = shift ? mul(c_inv, rpi[lg_split]) : c_inv;   // fold scalars of the unscaled vectors
        e->stats.host_ms += now_ms() - th;
        std::memcpy(&com_steps[6 * round], com, sizeof com); std::memcpy(&transcript[round], &c, sizeof c);
        prev_c = c;
        // folds (gipa.rs:262-290): hi = upper half, lo = lower half for all four vectors
        const double tf = now_ms();
        rc = fork_join_folds(e, [&]() -> int32_t {
            int32_t r2;
            if (batch && v.pA.ready && v.pB.ready) {                                  // same scalars and operands as the five calls below
                rq1[0].s = c; rq1[1].s = c; rq1[2].s = c_u; rq2[0].s = c_inv; rq2[1].s = c_inv_u;
                if ((r2 = fold_batch_dev<Fp>(e, e->stream2, rq1, shift ? 3 : 2, split))) return r2;
                return fold_batch_dev<Fp2>(e, e->stream, rq2, 2, split);
            }
            if ((r2 = fold_dev<Fp>(e, e->stream2, A + split, A, split, c, v.jac1, v.qt2, v.A2.as<G1A>(), &v.pA))) return r2;          // m_a  <- m_a_1 * c + m_a_2
            if (shift && (r2 = fold_dev<Fp>(e, e->stream4, AL + split, AL, split, c_u, v.jac1u, v.qt2, v.AU2.as<G1A>(), &v.pAU))) return r2;   // unscaled twin of m_a
            if ((r2 = fold_dev<Fp>(e, e->stream3, KB + split, KB, split, c, v.jac1b, v.qt2, v.KB2.as<G1A>(), &v.pKB))) return r2;       // ck_b <- ck_b_1 * c + ck_b_2
            if ((r2 = fold_dev<Fp2>(e, e->stream, B + split, B, split, c_inv, v.jac2, e->qtab, v.B2.as<G2A>(), &v.pB))) return r2;     // m_b  <- m_b_2 * c_inv + m_b_1
            // the precomputed-base form has its own scratch per vector, so the second G2 fold runs beside the first; the others share e->qtab
            hipStream_t st_ka = (v.pKA.ready && split <= e->cfg.pub.vm_fold_max) ? e->stream5 : e->stream;
            return fold_dev<Fp2>(e, st_ka, KA + split, KA, split, c_inv_u, v.jac2b, e->qtab, v.KA2.as<G2A>(), &v.pKA);                   // ck_a <- ck_a_2 * c_inv + ck_a_1
        });
        if (rc) return rc;
        e->stats.fold_ms += now_ms() - tf;
        std::swap(v.A, v.A2); std::swap(v.KB, v.KB2); std::swap(v.B, v.B2); std::swap(v.KA, v.KA2); if (shift) std::swap(v.AU, v.AU2);
        len = split; ++round;
    }
    HIPCHK(hipMemcpy(&ha, v.A.p, sizeof ha, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(&hkb, v.KB.p, sizeof hkb, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&hb, v.B.p, sizeof hb, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(&hka, v.KA.p, sizeof hka, hipMemcpyDeviceToHost));
    return RIPP_OK;
}

// upload the four projective inputs of a TIPP instance and normalise them into v
static int32_t tipp_upload(Engine* e, TippVecs& v, const ripp_g1j* m_a, const ripp_g2j* m_b, const ripp_g2j* ck_a, const ripp_g1j* ck_b, size_t n) {
    int32_t rc; if ((rc = v.reserve(n))) return rc;
    HIPCHK(hipMemcpyAsync(v.jac1.p, m_a, n * sizeof(G1J), hipMemcpyHostToDevice, e->stream)); if ((rc = e->normalize_dev<Fp>(v.jac1.as<G1J>(), n, v.A.as<G1A>()))) return rc; if ((rc = e->sync())) return rc;
    HIPCHK(hipMemcpyAsync(v.jac1.p, ck_b, n * sizeof(G1J), hipMemcpyHostToDevice, e->stream)); if ((rc = e->normalize_dev<Fp>(v.jac1.as<G1J>(), n, v.KB.as<G1A>()))) return rc; if ((rc = e->sync())) return rc;
    HIPCHK(hipMemcpyAsync(v.jac2.p, m_b, n * sizeof(G2J), hipMemcpyHostToDevice, e->stream)); if ((rc = e->normalize_dev<Fp2>(v.jac2.as<G2J>(), n, v.B.as<G2A>()))) return rc; if ((rc = e->sync())) return rc;
    HIPCHK(hipMemcpyAsync(v.jac2.p, ck_a, n * sizeof(G2J), hipMemcpyHostToDevice, e->stream)); if ((rc = e->normalize_dev<Fp2>(v.jac2.as<G2J>(), n, v.KA.as<G2A>()))) return rc; return e->sync();
}

API int32_t ripp_gipa_tipp_prove(const ripp_g1j* m_a, const ripp_g2j* m_b, const ripp_g2j* ck_a, const ripp_g1j* ck_b, size_t n,
                                 ripp_gt* com_steps, ripp_fr* transcript, ripp_g1j* base_a, ripp_g2j* base_b,
                                 ripp_g2j* ck_base_a, ripp_g1j* ck_base_b, ripp_stats* st) {
    if (n == 0 || (n & (n - 1))) return RIPP_ERR_POW2;                       // assert!(m_a.len().is_power_of_two()), gipa.rs:195
    LOCK; ENGINE;
    if (!m_a || !m_b || !ck_a || !ck_b || !base_a || !base_b || !ck_base_a || !ck_base_b || (n > 1 && (!com_steps || !transcript))) return RIPP_ERR_ARG;
    e->stats = ripp_stats{};
    const double t_start = now_ms();
    int32_t rc;
    G1A ha, hkb; G2A hb, hka;
    // ripp_config.n_devices = D > 1: the proof runs as D in-process ranks, one host thread and engine per device, vectors sharded by index residue as across
    // processes (element i on rank i mod D), the per-round exchange a copy through LocalComm (comm_core.inc) -- the unmodified single-process caller of the fused
    // prover reaches every device it drives.  D is rounded down to a power of two; shards below 1 024 elements are not worth a device.
    std::vector<DevSlot> sl;
    if ((rc = device_slots(e, n, 1024, &sl))) return rc;
    size_t D = 1; while (2 * D <= sl.size()) D *= 2;
    if (D > 1) {
        sl.resize(D); g_last_slots = (int32_t)D;
        LocalComm lc; lc.world = (int)D;
        const size_t nl = n / D, rounds = log2_sz(n);
        struct Out { std::vector<ripp_gt> steps; std::vector<ripp_fr> tr; G1A ha, hkb; G2A hb, hka; };
        std::vector<Out> outs(D);
        rc = run_on_devices(e, sl, [&](Engine* ee, size_t, size_t, int d) -> int32_t {
            t_lcomm = &lc; t_lrank = d;
            struct Unbind { ~Unbind() { t_lcomm = nullptr; t_lrank = 0; } } unbind;
            int32_t r2;
            {
                TippVecs v(false);
                // this rank's residue class of the four vectors, gathered on the host (the slices are the caller's: one strided pass each)
                std::vector<G1J> s1(nl); std::vector<G2J> s2(nl);
                auto up1 = [&](const ripp_g1j* src, DevBuf& dst) -> int32_t { for (size_t i = 0; i < nl; ++i) std::memcpy(&s1[i], &src[i * D + (size_t)d], sizeof(G1J));
                    HIPCHK(hipMemcpyAsync(v.jac1.p, s1.data(), nl * sizeof(G1J), hipMemcpyHostToDevice, ee->stream)); int32_t r3 = ee->normalize_dev<Fp>(v.jac1.as<G1J>(), nl, dst.as<G1A>()); return r3 ? r3 : ee->sync(); };
                auto up2 = [&](const ripp_g2j* src, DevBuf& dst) -> int32_t { for (size_t i = 0; i < nl; ++i) std::memcpy(&s2[i], &src[i * D + (size_t)d], sizeof(G2J));
                    HIPCHK(hipMemcpyAsync(v.jac2.p, s2.data(), nl * sizeof(G2J), hipMemcpyHostToDevice, ee->stream)); int32_t r3 = ee->normalize_dev<Fp2>(v.jac2.as<G2J>(), nl, dst.as<G2A>()); return r3 ? r3 : ee->sync(); };
                Out& o = outs[(size_t)d]; o.steps.resize(6 * std::max<size_t>(rounds, 1)); o.tr.resize(std::max<size_t>(rounds, 1));
                ShardCtx sc; sc.rank = d; sc.world = (int)D;
                if ((r2 = v.reserve(nl)) || (r2 = up1(m_a, v.A)) || (r2 = up1(ck_b, v.KB)) || (r2 = up2(m_b, v.B)) || (r2 = up2(ck_a, v.KA))
                    || (r2 = gipa_tipp_core(ee, v, nl, o.steps.data(), o.tr.data(), o.ha, o.hb, o.hka, o.hkb, nullptr, sc))) { lc.fail(); return r2; }
            }
            return RIPP_OK; });
        if (rc) return rc;
        for (size_t d = 1; d < D; ++d)          // every rank derives the same transcript from the same exchanged values
            if (std::memcmp(outs[d].tr.data(), outs[0].tr.data(), rounds * sizeof(ripp_fr))) { set_err("in-process ranks: the devices' transcripts differ"); return RIPP_ERR_DEVICE; }
        if (rounds) { std::memcpy(com_steps, outs[0].steps.data(), 6 * rounds * sizeof(ripp_gt)); std::memcpy(transcript, outs[0].tr.data(), rounds * sizeof(ripp_fr)); }
        ha = outs[0].ha; hkb = outs[0].hkb; hb = outs[0].hb; hka = outs[0].hka;
    } else {
        g_last_slots = 1;
        TippVecs v;
        if ((rc = tipp_upload(e, v, m_a, m_b, ck_a, ck_b, n))) return rc;
        if ((rc = gipa_tipp_core(e, v, n, com_steps, transcript, ha, hb, hka, hkb))) return rc;
    }
    const G1J ja = to_jac(ha), jkb = to_jac(hkb); const G2J jb = to_jac(hb), jka = to_jac(hka);
    std::memcpy(base_a, &ja, sizeof ja); std::memcpy(base_b, &jb, sizeof jb); std::memcpy(ck_base_a, &jka, sizeof jka); std::memcpy(ck_base_b, &jkb, sizeof jkb);
    return finish_stats(e, t_start, st, false);
}

// GIPA / TIPP across the communicator's ranks: every vector argument is this rank's shard (local j <-> global j * world + rank)
API int32_t ripp_gipa_tipp_prove_sharded(const ripp_g1j* m_a, const ripp_g2j* m_b, const ripp_g2j* ck_a, const ripp_g1j* ck_b, size_t n_local,
                                         ripp_gt* com_steps, ripp_fr* transcript, ripp_g1j* base_a, ripp_g2j* base_b,
                                         ripp_g2j* ck_base_a, ripp_g1j* ck_base_b, ripp_stats* st) {
    if (n_local == 0 || (n_local & (n_local - 1))) return RIPP_ERR_POW2;
    LOCK; ENGINE;
    comm_mark_proof();
    const ShardCtx sc = ShardCtx::from_comm();
    if (sc.world & (sc.world - 1)) { set_err("the number of ranks must be a power of two"); return RIPP_ERR_POW2; }
    if (!m_a || !m_b || !ck_a || !ck_b || !base_a || !base_b || !ck_base_a || !ck_base_b || (n_local * (size_t)sc.world > 1 && (!com_steps || !transcript))) return RIPP_ERR_ARG;
    e->stats = ripp_stats{};
    const double t_start = now_ms();
    TippVecs v; int32_t rc;
    if ((rc = tipp_upload(e, v, m_a, m_b, ck_a, ck_b, n_local))) return rc;
    G1A ha, hkb; G2A hb, hka;
    if ((rc = gipa_tipp_core(e, v, n_local, com_steps, transcript, ha, hb, hka, hkb, nullptr, sc))) return rc;
    const G1J ja = to_jac(ha), jkb = to_jac(hkb); const G2J jb = to_jac(hb), jka = to_jac(hka);
    std::memcpy(base_a, &ja, sizeof ja); std::memcpy(base_b, &jb, sizeof jb); std::memcpy(ck_base_a, &jka, sizeof jka); std::memcpy(ck_base_b, &jkb, sizeof jkb);
    return finish_stats(e, t_start, st, false);
}

// ---- TIPA: SRS handle, KZG openings (ip_proofs/src/tipa/mod.rs) ---------------------------------------------------------
struct ripp_srs { DevBuf gap, hbp; size_t num = 0; };   // normalised g_alpha_powers / h_beta_powers, resident in HBM

API int32_t ripp_srs_create(const ripp_g1j* g_alpha_powers, const ripp_g2j* h_beta_powers, size_t num, ripp_srs** out) {
    LOCK; ENGINE; if (!g_alpha_powers || !h_beta_powers || !out || !(num & 1)) return RIPP_ERR_ARG;
    const size_t n = (num + 1) / 2; if (n & (n - 1)) return RIPP_ERR_POW2;
    ripp_srs* s = new ripp_srs(); s->num = num;
    int32_t rc; G1J* dj1; G2J* dj2;
    if ((rc = s->gap.reserve(num * sizeof(G1A))) || (rc = s->hbp.reserve(num * sizeof(G2A))) ||
        (rc = upload<G1J>(e, e->jacG1, g_alpha_powers, num, &dj1)) || (rc = e->normalize_dev<Fp>(dj1, num, s->gap.as<G1A>())) ||
        (rc = upload<G2J>(e, e->jacG2, h_beta_powers, num, &dj2)) || (rc = e->normalize_dev<Fp2>(dj2, num, s->hbp.as<G2A>())) || (rc = e->sync())) {
        s->gap.release(); s->hbp.release(); delete s; return rc;
    }
    ++g_live_handles;
    *out = s; return RIPP_OK;
}
API void ripp_srs_destroy(ripp_srs* s) { if (!s) return; LOCK; s->gap.release(); s->hbp.release(); delete s; --g_live_handles; }

extern "C++" {
// structured_generators_scalar_power (tipa/mod.rs:372-391): the powers s^i are a sequential host recurrence, the num scalar
// multiplications of the one generator run on the device
template <class F> static int32_t srs_powers(const Affine<F>& g, const ripp_fr* s_in, size_t num, void* out) {
    LOCK; ENGINE; if (!s_in || (num && !out)) return RIPP_ERR_ARG; if (!num) return RIPP_OK;
    Fr s; std::memcpy(&s, s_in, sizeof s);
    const std::vector<Fr> pw = fr_powers(s, num);
    DevBuf& jac = std::is_same<F, Fp>::value ? e->jacG1 : e->jacG2; DevBuf& aff = std::is_same<F, Fp>::value ? e->affG1 : e->affG2;
    int32_t rc; Fr* dk;
    if ((rc = upload<Fr>(e, e->tmpR, pw.data(), num, &dk)) || (rc = jac.reserve(num * sizeof(Jac<F>))) || (rc = aff.reserve(sizeof(Affine<F>)))) return rc;
    HIPCHK(hipMemcpyAsync(aff.p, &g, sizeof g, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scale_pts<F>), dim3(nblk(num, 256)), dim3(256), 0, e->stream, aff.as<Affine<F>>(), 0u, dk, (uint32_t)num, jac.as<Jac<F>>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, jac.p, num * sizeof(Jac<F>), hipMemcpyDeviceToHost, e->stream));
    return e->sync();
}

// polynomial_coefficients_from_transcript (tipa/mod.rs:406-422) before the zero interleave: co[j] multiplies X^(2j)
static std::vector<Fr> ck_poly_coeffs(const std::vector<Fr>& tr, const Fr& r_shift) {
    std::vector<Fr> co((size_t)1 << tr.size()); co[0] = Fr::one(); Fr p2r = r_shift; size_t cnt = 1;
    for (size_t i = 0; i < tr.size(); ++i) {
        const Fr xr = mul(tr[i], p2r);
        for (size_t j = 0; j < ((size_t)1 << i); ++j) co[cnt + j] = mul(co[j], xr);
        cnt += (size_t)1 << i; p2r = mul(p2r, p2r);
    }
    return co;
}
// prove_commitment_key_kzg_opening (tipa/mod.rs:304-337): quotient of p(X) - p(c) by (X - c) by synthetic division on the
// host (O(n) Fr products); the 2n-1 term MSM against the resident SRS powers then runs on the device
static int32_t kzg_quotient(const std::vector<Fr>& tr, const Fr& r_shift, const Fr& c, size_t num, std::vector<Fr>& q) {
    const std::vector<Fr> co = ck_poly_coeffs(tr, r_shift);
    if (2 * co.size() - 1 != num) { set_err("SRS size does not match the transcript length (assert_eq! at tipa/mod.rs:313)"); return RIPP_ERR_ARG; }
    q.assign(num, Fr::zero());
    Fr carry = Fr::zero();
    for (size_t k = num - 1; k >= 1; --k) {                       // q[k-1] = p[k] + c q[k];  p[k] = co[k/2] for even k, else 0
        Fr t = mul(carry, c); if (!(k & 1)) t = add(t, co[k >> 1]);
        q[k - 1] = t; carry = t;
    }
    return RIPP_OK;
}
// sharded: the SRS is resident in FULL on every GPU (2n-1 points: 600 MB at n = 2^20), the WORK is split -- rank w sums the terms
// k = w (mod world): its residue class of the powers is gathered contiguously on the device, its quotient coefficients on the host
template <class F> static int32_t kzg_opening_launch(Engine* e, int slot, hipStream_t st, const Affine<F>* powers, const std::vector<Fr>& q, const ShardCtx& sc = ShardCtx()) {
    int32_t rc;
    if (sc.world == 1) {
        if ((rc = e->kzg_q[slot].reserve(q.size() * sizeof(Fr)))) return rc;
        if ((rc = e->stage[slot].reserve(q.size() * sizeof(Fr)))) return rc;
        std::memcpy(e->stage[slot].p, q.data(), q.size() * sizeof(Fr));
        if ((rc = e->stage[slot].send(e->kzg_q[slot].p, q.size() * sizeof(Fr), st))) return rc;
        return e->msm_launch<F>(e->msm_scratch[slot], st, powers, e->kzg_q[slot].as<Fr>(), q.size());
    }
    const size_t cnt = q.size() > (size_t)sc.rank ? (q.size() - sc.rank + sc.world - 1) / sc.world : 0;
    if ((rc = e->stage[slot].reserve(std::max<size_t>(cnt, 1) * sizeof(Fr)))) return rc;
    Fr* const mine = e->stage[slot].as<Fr>(); for (size_t j = 0; j < cnt; ++j) mine[j] = q[sc.rank + j * (size_t)sc.world];
    if ((rc = e->kzg_q[slot].reserve(std::max<size_t>(cnt, 1) * sizeof(Fr))) || (rc = e->kzg_bases[slot].reserve(std::max<size_t>(cnt, 1) * sizeof(Affine<F>)))) return rc;
    if (cnt) {
        if ((rc = e->stage[slot].send(e->kzg_q[slot].p, cnt * sizeof(Fr), st))) return rc;
        HIPCHK(hipMemcpy2DAsync(e->kzg_bases[slot].p, sizeof(Affine<F>), powers + sc.rank, (size_t)sc.world * sizeof(Affine<F>), sizeof(Affine<F>), cnt, hipMemcpyDeviceToDevice, st));
    }
    return e->msm_launch<F>(e->msm_scratch[slot], st, e->kzg_bases[slot].as<Affine<F>>(), e->kzg_q[slot].as<Fr>(), cnt);
}
template <class F> static int32_t kzg_opening_dev(Engine* e, const Affine<F>* powers, size_t num, const std::vector<Fr>& tr, const Fr& r_shift, const Fr& c, Jac<F>* out, const ShardCtx& sc = ShardCtx()) {
    std::vector<Fr> q; int32_t rc;
    if ((rc = kzg_quotient(tr, r_shift, c, num, q)) || (rc = kzg_opening_launch<F>(e, 0, e->stream, powers, q, sc)) || (rc = e->sync())) return rc;
    *out = *reinterpret_cast<const Jac<F>*>(e->msm_scratch[0].host_out);
    return shard_add_pts<F>(e, sc, out, 1);
}
}  // extern "C++"
API int32_t ripp_srs_powers_g1(const ripp_fr* s, size_t num, ripp_g1j* out) { return srs_powers<Fp>(g1_generator(), s, num, out); }
API int32_t ripp_srs_powers_g2(const ripp_fr* s, size_t num, ripp_g2j* out) { return srs_powers<Fp2>(g2_generator(), s, num, out); }

extern "C++" {
// strided device gather of the even SRS powers (get_commitment_keys, tipa/mod.rs:114-118)
template <class T> static int32_t gather_even(Engine* e, const T* src, size_t n, T* dst) {
    HIPCHK(hipMemcpy2DAsync(dst, sizeof(T), src, 2 * sizeof(T), sizeof(T), n, hipMemcpyDeviceToDevice, e->stream)); return RIPP_OK;
}
}
API int32_t ripp_srs_commitment_keys(const ripp_srs* s, ripp_g2j* ck_1, ripp_g1j* ck_2) {
    LOCK; ENGINE; if (!s || !ck_1 || !ck_2) return RIPP_ERR_ARG;
    const size_t n = (s->num + 1) / 2; int32_t rc;
    if ((rc = e->affG1.reserve(n * sizeof(G1A))) || (rc = e->affG2.reserve(n * sizeof(G2A)))) return rc;
    if ((rc = gather_even<G2A>(e, const_cast<ripp_srs*>(s)->hbp.as<G2A>(), n, e->affG2.as<G2A>())) || (rc = gather_even<G1A>(e, const_cast<ripp_srs*>(s)->gap.as<G1A>(), n, e->affG1.as<G1A>()))) return rc;
    std::vector<G1A> h1(n); std::vector<G2A> h2(n);
    HIPCHK(hipMemcpyAsync(h1.data(), e->affG1.p, n * sizeof(G1A), hipMemcpyDeviceToHost, e->stream)); HIPCHK(hipMemcpyAsync(h2.data(), e->affG2.p, n * sizeof(G2A), hipMemcpyDeviceToHost, e->stream));
    if ((rc = e->sync())) return rc;
    G1J* o1 = reinterpret_cast<G1J*>(ck_2); G2J* o2 = reinterpret_cast<G2J*>(ck_1);
    for (size_t i = 0; i < n; ++i) { o1[i] = to_jac(h1[i]); o2[i] = to_jac(h2[i]); }
    return RIPP_OK;
}

// the KZG half of TIPA::prove_with_srs_shift (tipa/mod.rs:186-223) once GIPA has produced transcript and final keys
static int32_t tipp_kzg(Engine* e, const ripp_srs* srs, const ripp_fr* transcript, size_t rounds, const Fr& r_shift, const G2A& hka, const G1A& hkb,
                        G2J* opening_a, G1J* opening_b, Fr* kzg_c, const ShardCtx& sc = ShardCtx()) {
    std::vector<Fr> tr(rounds), tri(rounds);
    for (size_t i = 0; i < rounds; ++i) { std::memcpy(&tr[i], &transcript[rounds - 1 - i], sizeof(Fr)); tri[i] = inv(tr[i]); }   // aux.r_transcript and its inverses, :190-191
    const Fr r_inv = inv(r_shift);                                                                                          // :192
    const Fr c = fs::kzg_challenge(tr[0], hka, &hkb);                                                                       // :194-209
    ripp_srs* s = const_cast<ripp_srs*>(srs); int32_t rc;
    // the two openings are independent: quotients on two host threads, MSMs side by side on two streams
    std::vector<Fr> qa, qb;
    auto fb = host_pool().submit([&]() { return kzg_quotient(tr, Fr::one(), c, s->num, qb); });
    rc = kzg_quotient(tri, r_inv, c, s->num, qa); const int32_t rcb = fb.get();
    if (rc || rcb) return rc ? rc : rcb;
    if ((rc = kzg_opening_launch<Fp2>(e, 0, e->stream, s->hbp.as<G2A>(), qa, sc))) return rc;                                 // :212-217
    if ((rc = kzg_opening_launch<Fp>(e, 1, e->stream3, s->gap.as<G1A>(), qb, sc))) return rc;                                  // :218-223
    if ((rc = e->sync())) return rc; HIPCHK(hipStreamSynchronize(e->stream3));
    *opening_a = *reinterpret_cast<const G2J*>(e->msm_scratch[0].host_out); *opening_b = *reinterpret_cast<const G1J*>(e->msm_scratch[1].host_out);
    if ((rc = shard_add_pts<Fp2>(e, sc, opening_a, 1)) || (rc = shard_add_pts<Fp>(e, sc, opening_b, 1))) return rc;
    *kzg_c = c; return RIPP_OK;
}

API int32_t ripp_tipa_tipp_prove(const ripp_srs* srs, const ripp_g1j* m_a, const ripp_g2j* m_b, const ripp_g2j* ck_a, const ripp_g1j* ck_b, size_t n,
                                 const ripp_fr* r_shift, ripp_gt* com_steps, ripp_fr* transcript, ripp_g1j* base_a, ripp_g2j* base_b,
                                 ripp_g2j* final_ck_a, ripp_g1j* final_ck_b, ripp_g2j* opening_a, ripp_g1j* opening_b, ripp_fr* kzg_challenge, ripp_stats* st) {
    if (n < 2 || (n & (n - 1))) return RIPP_ERR_POW2;                        // n = 1 would unwrap an empty transcript (tipa/mod.rs:200-202)
    LOCK; ENGINE;
    if (!srs || !m_a || !m_b || !ck_a || !ck_b || !r_shift || !com_steps || !transcript || !base_a || !base_b || !final_ck_a || !final_ck_b || !opening_a || !opening_b || !kzg_challenge) return RIPP_ERR_ARG;
    if (srs->num != 2 * n - 1) { set_err("SRS holds " + std::to_string(srs->num) + " powers, need 2n-1 = " + std::to_string(2 * n - 1)); return RIPP_ERR_ARG; }
    e->stats = ripp_stats{};
    const double t_start = now_ms();
    TippVecs v; int32_t rc;
    if ((rc = tipp_upload(e, v, m_a, m_b, ck_a, ck_b, n))) return rc;
    G1A ha, hkb; G2A hb, hka;
    if ((rc = gipa_tipp_core(e, v, n, com_steps, transcript, ha, hb, hka, hkb))) return rc;
    const size_t rounds = log2_sz(n);
    Fr rs; std::memcpy(&rs, r_shift, sizeof rs);
    G2J oa; G1J ob; Fr c;
    if ((rc = tipp_kzg(e, srs, transcript, rounds, rs, hka, hkb, &oa, &ob, &c))) return rc;
    const G1J ja = to_jac(ha), jkb = to_jac(hkb); const G2J jb = to_jac(hb), jka = to_jac(hka);
    std::memcpy(base_a, &ja, sizeof ja); std::memcpy(base_b, &jb, sizeof jb); std::memcpy(final_ck_a, &jka, sizeof jka); std::memcpy(final_ck_b, &jkb, sizeof jkb);
    std::memcpy(opening_a, &oa, sizeof oa); std::memcpy(opening_b, &ob, sizeof ob); std::memcpy(kzg_challenge, &c, sizeof c);
    return finish_stats(e, t_start, st, false);
}

// ---- TIPAWithSSM (MIPP with a structured scalar vector), ip_proofs/src/tipa/structured_scalar_message.rs ------------------
struct SsmVecs {
    DevBuf A, A2, S, S2, KA, KA2, jac1, jac2, qt2;
    FoldPre pA, pKA;                        // second fold bases of the small rounds
    VecLease lease{&g_ssm_cache, {&A, &A2, &S, &S2, &KA, &KA2, &jac1, &jac2, &qt2, &pA.pow_h, &pA.parts, &pKA.pow_h, &pKA.parts}};      // (last member)
    int32_t reserve(size_t n) {
        int32_t rc;
        if ((rc = A.reserve(n * sizeof(G1A))) || (rc = A2.reserve(n * sizeof(G1A))) || (rc = S.reserve(n * sizeof(Fr))) || (rc = S2.reserve(n * sizeof(Fr))) ||
            (rc = KA.reserve(n * sizeof(G2A))) || (rc = KA2.reserve(n * sizeof(G2A))) || (rc = jac1.reserve(n * sizeof(G1J))) || (rc = jac2.reserve(n * sizeof(G2J)))) return rc;
        return RIPP_OK;
    }
};

// the message of a second-tier argument: n projective G1 points of the host, normalised into v.A (v reserved for n)
static int32_t ssm_load_message(Engine* e, SsmVecs& v, const ripp_g1j* m, size_t n) {
    HIPCHK(hipMemcpyAsync(v.jac1.p, m, n * sizeof(G1J), hipMemcpyHostToDevice, e->stream));
    return e->normalize_dev<Fp>(v.jac1.as<G1J>(), n, v.A.as<G1A>());
}
// GIPA<MultiexponentiationInnerProduct<G1>, AFGHO-G1, SSMPlaceholder, Identity<G1>>::_prove (gipa.rs:181-312): the rounds alone, which are all of
// GIPAWithSSM::prove_with_structured_scalar_message (ssm.rs:66-84; the second tier of the transparent polynomial commitment, tpc_api.inc).
// Per round: two pairing products share one line launch, two G1 MSMs over the halves.  Steps and transcript in ROUND order; *rounds_out = their number.
static int32_t tipa_ssm_rounds(Engine* e, SsmVecs& v, size_t n, ripp_gt* com_gt, ripp_g1j* com_g1, ripp_fr* transcript,
                               G1A& ha, Fr& hs, G2A& hka, size_t* rounds_out, ShardCtx sc = ShardCtx()) {
    int32_t rc;
    size_t len = n, round = 0;                 // n = LOCAL length
    Fr prev_c = Fr::zero();
    std::vector<Fp12> rows(2 * N_LINES);
    for (;;) {
        if (len == 1) {
            if (sc.world == 1) break;
            if ((rc = shard_gather_tail<G1A>(e, sc, v.A)) || (rc = shard_gather_tail<Fr>(e, sc, v.S)) || (rc = shard_gather_tail<G2A>(e, sc, v.KA))) return rc;
            len = (size_t)sc.world; sc.world = 1;
            if ((rc = v.reserve(len))) return rc;
            continue;
        }
        const size_t split = len / 2;
        const G1A* A = v.A.as<G1A>(); const G2A* KA = v.KA.as<G2A>(); const Fr* S = v.S.as<Fr>();
        const G1A* as[2] = {A + split, A}; const G2A* bs[2] = {KA, KA + split};     // com_1.0 = (m_a_1, ck_a_1), com_2.0 = (m_a_2, ck_a_2)   gipa.rs:209-231
        const double tp = now_ms();
        // the two inner products of the round run on their own streams beside the pairing products (independent work)
        if ((rc = e->msm_launch<Fp>(e->msm_scratch[0], e->stream2, A + split, S, split))) return rc;           // IP::inner_product(m_a_1, m_b_1)
        if ((rc = e->msm_launch<Fp>(e->msm_scratch[1], e->stream3, A, S + split, split))) return rc;           // IP::inner_product(m_a_2, m_b_2)
        if ((rc = e->step_products(as, bs, 2, split, rows.data()))) return rc;
        HIPCHK(hipStreamSynchronize(e->stream2)); HIPCHK(hipStreamSynchronize(e->stream3));
        G1J ip[2] = {*reinterpret_cast<const G1J*>(e->msm_scratch[0].host_out), *reinterpret_cast<const G1J*>(e->msm_scratch[1].host_out)};
        if ((rc = shard_add_pts<Fp>(e, sc, ip, 2))) return rc;                                                    // partial MSM sums -> sums
        if ((rc = fold_precompute<Fp>(e, e->stream2, A + split, split, v.pA)) || (rc = fold_precompute<Fp2>(e, e->stream, KA + split, split, v.pKA))) return rc;   // small rounds: during the host phase
        e->stats.miller_products_ms += now_ms() - tp;
        const double th = now_ms();
        Fp12 gt[2];
        if (sc.world > 1) {
            { auto fut = host_pool().submit([&rows]() { return miller_combine(rows.data() + N_LINES); }); gt[0] = miller_combine(rows.data()); gt[1] = fut.get(); }
            if ((rc = shard_mul_gt(e, sc, gt, 2))) return rc;
            const Fp12 m1 = gt[1];
            auto fut = host_pool().submit([m1]() { return final_exponentiation(m1); }); gt[0] = final_exponentiation(gt[0]); gt[1] = fut.get();
        } else
        { auto fut = host_pool().submit([&rows]() { return final_exponentiation(miller_combine(rows.data() + N_LINES)); });
          gt[0] = final_exponentiation(miller_combine(rows.data())); gt[1] = fut.get(); }
        const G1A ipa[2] = {to_affine(ip[0]), to_affine(ip[1])};
        Fr c_inv; const Fr c = fs::gipa_challenge(round ? &prev_c : nullptr, fs::Com{gt[0], fs::SSMPlaceholder{}, ipa[0]}, fs::Com{gt[1], fs::SSMPlaceholder{}, ipa[1]}, c_inv);
        e->stats.host_ms += now_ms() - th;
        std::memcpy(&com_gt[2 * round], gt, sizeof gt); std::memcpy(&com_g1[2 * round], ip, sizeof ip); std::memcpy(&transcript[round], &c, sizeof c);
        prev_c = c;
        const double tf = now_ms();
        rc = fork_join_folds(e, [&]() -> int32_t {
            int32_t r2;
            if ((r2 = fold_dev<Fp>(e, e->stream2, A + split, A, split, c, v.jac1, v.qt2, v.A2.as<G1A>(), &v.pA))) return r2;       // m_a  <- m_a_1 * c + m_a_2
            hipLaunchKernelGGL(k_fold_fr, dim3(nblk(split, 256)), dim3(256), 0, e->stream3, S + split, S, (uint32_t)split, c_inv, v.S2.as<Fr>());   // m_b  <- m_b_2 * c_inv + m_b_1
            HIPCHK(hipGetLastError());
            return fold_dev<Fp2>(e, e->stream, KA + split, KA, split, c_inv, v.jac2, e->qtab, v.KA2.as<G2A>(), &v.pKA);              // ck_a <- ck_a_2 * c_inv + ck_a_1
        });
        if (rc) return rc;
        e->stats.fold_ms += now_ms() - tf;
        std::swap(v.A, v.A2); std::swap(v.S, v.S2); std::swap(v.KA, v.KA2);
        len = split; ++round;
    }
    HIPCHK(hipMemcpy(&ha, v.A.p, sizeof ha, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(&hs, v.S.p, sizeof hs, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(&hka, v.KA.p, sizeof hka, hipMemcpyDeviceToHost));
    *rounds_out = round; return RIPP_OK;
}
// the rounds above + the KZG opening of ck_a (ssm.rs:225-254)
static int32_t tipa_ssm_core(Engine* e, const ripp_srs* srs, SsmVecs& v, size_t n, ripp_gt* com_gt, ripp_g1j* com_g1, ripp_fr* transcript,
                             G1A& ha, Fr& hs, G2A& hka, G2J* opening_a, Fr* kzg_c, ShardCtx sc = ShardCtx()) {
    const ShardCtx sc0 = sc;                   // the KZG opening is sharded by the ORIGINAL partition
    int32_t rc; size_t rounds = 0;
    if ((rc = tipa_ssm_rounds(e, v, n, com_gt, com_g1, transcript, ha, hs, hka, &rounds, sc))) return rc;
    std::vector<Fr> tri(rounds);
    for (size_t i = 0; i < rounds; ++i) { Fr t; std::memcpy(&t, &transcript[rounds - 1 - i], sizeof t); tri[i] = inv(t); }         // ssm.rs:227-229
    Fr first; std::memcpy(&first, &transcript[rounds - 1], sizeof first);
    if (trace_on()) fprintf(stderr, "[ripp] ssm: GIPA rounds done (products+msm %.1f ms, host %.1f ms, folds %.1f ms cumulative)\n", e->stats.miller_products_ms, e->stats.host_ms, e->stats.fold_ms);
    const Fr c = fs::kzg_challenge(first, hka, nullptr);                                                                           // ssm.rs:231-246
    ripp_srs* s = const_cast<ripp_srs*>(srs);
    if ((rc = kzg_opening_dev<Fp2>(e, s->hbp.as<G2A>(), s->num, tri, Fr::one(), c, opening_a, sc0))) return rc;                      // ssm.rs:249-254
    *kzg_c = c; return RIPP_OK;
}

API int32_t ripp_tipa_ssm_prove(const ripp_srs* srs, const ripp_g1j* m_a, const ripp_fr* m_b, const ripp_g2j* ck_a, size_t n,
                                ripp_gt* com_gt, ripp_g1j* com_g1, ripp_fr* transcript, ripp_g1j* base_a, ripp_fr* base_b,
                                ripp_g2j* final_ck_a, ripp_g2j* opening_a, ripp_fr* kzg_challenge, ripp_stats* st) {
    if (n < 2 || (n & (n - 1))) return RIPP_ERR_POW2;
    LOCK; ENGINE;
    if (!srs || !m_a || !m_b || !ck_a || !com_gt || !com_g1 || !transcript || !base_a || !base_b || !final_ck_a || !opening_a || !kzg_challenge) return RIPP_ERR_ARG;
    if (srs->num != 2 * n - 1) { set_err("SRS holds " + std::to_string(srs->num) + " powers, need 2n-1 = " + std::to_string(2 * n - 1)); return RIPP_ERR_ARG; }
    e->stats = ripp_stats{};
    const double t_start = now_ms();
    SsmVecs v; int32_t rc; if ((rc = v.reserve(n)) || (rc = ssm_load_message(e, v, m_a, n))) return rc;
    HIPCHK(hipMemcpyAsync(v.jac2.p, ck_a, n * sizeof(G2J), hipMemcpyHostToDevice, e->stream)); if ((rc = e->normalize_dev<Fp2>(v.jac2.as<G2J>(), n, v.KA.as<G2A>()))) return rc;
    HIPCHK(hipMemcpyAsync(v.S.p, m_b, n * sizeof(Fr), hipMemcpyHostToDevice, e->stream)); if ((rc = e->sync())) return rc;
    G1A ha; Fr hs; G2A hka; G2J oa; Fr c;
    if ((rc = tipa_ssm_core(e, srs, v, n, com_gt, com_g1, transcript, ha, hs, hka, &oa, &c))) return rc;
    const G1J ja = to_jac(ha); const G2J jka = to_jac(hka);
    std::memcpy(base_a, &ja, sizeof ja); std::memcpy(base_b, &hs, sizeof hs); std::memcpy(final_ck_a, &jka, sizeof jka); std::memcpy(opening_a, &oa, sizeof oa); std::memcpy(kzg_challenge, &c, sizeof c);
    return finish_stats(e, t_start, st, false);
}

// ---- Groth16 aggregation: aggregate_proofs (ip_proofs/src/applications/groth16_aggregation.rs:77-160) ---------------------
static_assert(sizeof(ripp_aggregate_proof) == 4 * sizeof(Fp12) + sizeof(G1J) + sizeof(Fr) + 2 * sizeof(void*) + 2 * (sizeof(G1J) + sizeof(G2J)) + sizeof(G2J) + sizeof(G1J) + sizeof(Fr)
              + 3 * sizeof(void*) + sizeof(G1J) + sizeof(Fr) + 2 * sizeof(G2J) + sizeof(Fr), "ripp_aggregate_proof layout");

// n = LOCAL number of proofs (this rank's shard: local j <-> global j * world + rank); sc.world == 1: the unsharded aggregation
static int32_t aggregate_impl(Engine* e, const ripp_srs* srs, const ripp_g1a* a, const ripp_g2a* b, const ripp_g1a* c, size_t n, ripp_aggregate_proof* out, ripp_stats* st, const ShardCtx sc) {
    const size_t n_glob = n * (size_t)sc.world;
    if (srs->num != 2 * n_glob - 1) { set_err("SRS holds " + std::to_string(srs->num) + " powers, need 2n-1 = " + std::to_string(2 * n_glob - 1)); return RIPP_ERR_ARG; }
    e->stats = ripp_stats{};
    const double t_start = now_ms();
    ripp_srs* s = const_cast<ripp_srs*>(srs);
    TippVecs v; SsmVecs w; DevBuf dCK1, dRv; int32_t rc;
    struct Cleanup { DevBuf &x, &y; ~Cleanup() { x.release(); y.release(); } } cleanup{dCK1, dRv};
    if ((rc = v.reserve(n)) || (rc = w.reserve(n)) || (rc = dCK1.reserve(n * sizeof(G2A))) || (rc = dRv.reserve(n * sizeof(Fr)))) return rc;
    // a -> v.A2 (unscaled), b -> v.B, c -> w.A;  ck_1 -> dCK1 and w.KA, ck_2 -> v.KB   (get_commitment_keys, tipa/mod.rs:114-118)
    HIPCHK(hipMemcpyAsync(v.A2.p, a, n * sizeof(G1A), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(v.B.p, b, n * sizeof(G2A), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(w.A.p, c, n * sizeof(G1A), hipMemcpyHostToDevice, e->stream));
    // key i = power 2 i of the SRS; this rank's keys i = j * world + rank are the powers 2 world j + 2 rank: one strided device gather
    HIPCHK(hipMemcpy2DAsync(dCK1.p, sizeof(G2A), s->hbp.as<G2A>() + 2 * sc.rank, 2 * (size_t)sc.world * sizeof(G2A), sizeof(G2A), n, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipMemcpy2DAsync(v.KB.p, sizeof(G1A), s->gap.as<G1A>() + 2 * sc.rank, 2 * (size_t)sc.world * sizeof(G1A), sizeof(G1A), n, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(w.KA.p, dCK1.p, n * sizeof(G2A), hipMemcpyDeviceToDevice, e->stream));
    std::vector<Fp12> rows(3 * N_LINES);
    // k products of the last step_products call -> GT values: this rank's Miller values, product over ranks, final exponentiations
    auto finish_all = [&](int cnt, Fp12* z) -> int32_t {
        std::vector<std::future<Fp12>> f;
        for (int k = 1; k < cnt; ++k) f.push_back(host_pool().submit([&rows, k]() { return miller_combine(rows.data() + (size_t)k * N_LINES); }));
        z[0] = miller_combine(rows.data()); for (int k = 1; k < cnt; ++k) z[k] = f[k - 1].get();
        int32_t r2 = shard_mul_gt(e, sc, z, cnt); if (r2) return r2;
        std::vector<std::future<Fp12>> g;
        for (int k = 1; k < cnt; ++k) { const Fp12 m = z[k]; g.push_back(host_pool().submit([m]() { return final_exponentiation(m); })); }
        z[0] = final_exponentiation(z[0]); for (int k = 1; k < cnt; ++k) z[k] = g[k - 1].get();
        return RIPP_OK; };
    {   // com_a = IP(a, ck_1), com_b = IP(ck_2, b), com_c = IP(c, ck_1): one line launch over three products   (:100-102)
        const G1A* as[3] = {v.A2.as<G1A>(), v.KB.as<G1A>(), w.A.as<G1A>()}; const G2A* bs[3] = {dCK1.as<G2A>(), v.B.as<G2A>(), dCK1.as<G2A>()};
        if ((rc = e->step_products(as, bs, 3, n, rows.data()))) return rc;
        Fp12 z[3]; if ((rc = finish_all(3, z))) return rc;
        std::memcpy(&out->com_a, &z[0], sizeof z[0]); std::memcpy(&out->com_b, &z[1], sizeof z[1]); std::memcpy(&out->com_c, &z[2], sizeof z[2]);
    }
    Fp12 com_a, com_b, com_c; std::memcpy(&com_a, &out->com_a, sizeof com_a); std::memcpy(&com_b, &out->com_b, sizeof com_b); std::memcpy(&com_c, &out->com_c, sizeof com_c);
    const Fr r = fs::aggregation_challenge(com_a, com_b, com_c);                                                        // :105-116
    std::memcpy(&out->r, &r, sizeof r);
    if (trace_on()) fprintf(stderr, "[ripp] aggregate: upload + 3 commitments done at t=%.1f ms\n", now_ms() - t_start);
    // r_vec = (1, r, r^2, ...) (:118)
    if ((rc = e->stage[2].reserve(n * sizeof(Fr)))) return rc;
    Fr* const rv = e->stage[2].as<Fr>();                                         // this rank's r^(j world + rank)
    { Fr step = Fr::one(), first = Fr::one();
      for (int w = 0; w < sc.world; ++w) step = mul(step, r);
      for (int w = 0; w < sc.rank; ++w) first = mul(first, r);
      rv[0] = first; for (size_t i = 1; i < n; ++i) rv[i] = mul(rv[i - 1], step); }
    if ((rc = e->stage[2].send(dRv.p, n * sizeof(Fr), e->stream))) return rc;
    HIPCHK(hipMemcpyAsync(w.S.p, dRv.p, n * sizeof(Fr), hipMemcpyDeviceToDevice, e->stream));
    // a_r = a_i * r^i (:119-123) -> v.A, with the unscaled a_i kept in v.AU.  ck_1_r = ck_1_i * r^-i (:127-131) is NOT materialised: the
    // TIPP core below runs in its implicit-shift form on the unscaled keys (see gipa_tipp_core), which removes the n G2 scalar
    // multiplications, and the sanity product of :133-136, IP(a_r, ck_1_r) == com_a, collapses to IP(a, ck_1) == com_a -- the very
    // product computed above -- so it holds by construction and is not recomputed.
    if ((rc = v.AU.reserve(n * sizeof(G1A))) || (rc = v.AU2.reserve(n * sizeof(G1A))) || (rc = v.jac1u.reserve(n * sizeof(G1J)))) return rc;
    HIPCHK(hipMemcpyAsync(v.AU.p, v.A2.p, n * sizeof(G1A), hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(v.KA.p, dCK1.p, n * sizeof(G2A), hipMemcpyDeviceToDevice, e->stream));
    if ((rc = e->scale_g1_dev(v.AU.as<G1A>(), 1u, dRv.as<Fr>(), n, v.jac1.as<G1J>()))) return rc;
    HIPCHK(hipGetLastError());
    if ((rc = e->normalize_dev<Fp>(v.jac1.as<G1J>(), n, v.A.as<G1A>()))) return rc;
    {   // ip_ab = IP(a_r, b) (:124)
        const G1A* as[1] = {v.A.as<G1A>()}; const G2A* bs[1] = {v.B.as<G2A>()};
        if ((rc = e->step_products(as, bs, 1, n, rows.data()))) return rc;
        Fp12 ip_ab; if ((rc = finish_all(1, &ip_ab))) return rc;
        std::memcpy(&out->ip_ab, &ip_ab, sizeof ip_ab);
    }
    if (trace_on()) fprintf(stderr, "[ripp] aggregate: scaling + ip_ab done at t=%.1f ms\n", now_ms() - t_start);
    G1J agg_c; if ((rc = e->msm_dev<Fp>(w.A.as<G1A>(), dRv.as<Fr>(), n, &agg_c)) || (rc = shard_add_pts<Fp>(e, sc, &agg_c, 1))) return rc;   // :125
    std::memcpy(&out->agg_c, &agg_c, sizeof agg_c);
    if (trace_on()) fprintf(stderr, "[ripp] aggregate: agg_c MSM done at t=%.1f ms\n", now_ms() - t_start);
    const size_t rounds = log2_sz(n_glob);
    // The two sub-proofs are independent (:138-149) and each is a chain of ~log2 n latency-bound rounds in which host and device take turns
    // waiting.  Unsharded, the TIPAWithSSM proof therefore runs on a second host thread with the engine's auxiliary streams and scratch
    // (Engine::aux_engine) BESIDE the TIPP proof: 68 + 55 ms -> ~max of the two at n = 2^14.  Sharded proofs run them side by side as well, their exchanges
    // paired by count in one all-gather (comm_core.inc: CommMux).  RIPP_AGG_SEQUENTIAL=1 keeps the sequence (A/B, and the parity test runs both).
    auto ssm_block = [&](Engine* ee) -> int32_t {   // tipa_proof_c = TIPAWithSSM::prove_with_structured_scalar_message(srs, (c, r_vec), ck_1)   (:145-149)
        int32_t r2; G1A ha; Fr hs; G2A hka; G2J oa; Fr kc;
        if ((r2 = tipa_ssm_core(ee, srs, w, n, out->c_com_gt, out->c_com_g1, out->c_transcript, ha, hs, hka, &oa, &kc, sc))) return r2;
        const G1J ja = to_jac(ha); const G2J jka = to_jac(hka);
        std::memcpy(&out->c_base_a, &ja, sizeof ja); std::memcpy(&out->c_base_b, &hs, sizeof hs); std::memcpy(&out->c_final_ck_a, &jka, sizeof jka);
        std::memcpy(&out->c_opening_a, &oa, sizeof oa); std::memcpy(&out->c_kzg_c, &kc, sizeof kc);
        return RIPP_OK; };
    Engine* e2 = !e->cfg.pub.agg_sequential ? e->aux_engine() : nullptr;
    // Sharded: both provers exchange through the ONE communicator, their k-th exchanges paired in one all-gather (comm_core.inc: CommMux) -- the order of
    // the collectives is then the same on every rank whatever the threads' timing (build round 4 ran the sub-proofs in sequence for that reason).
    const bool muxed = e2 && sc.world > 1;
    std::thread ssm_thread; int32_t ssm_rc = RIPP_OK; std::string ssm_err;
    bool tipp_done = false;
    struct Join { std::thread& t; bool mux; bool& done0; ~Join() { if (mux && !done0) mux_done(0, RIPP_ERR_DEVICE); if (t.joinable()) t.join(); if (mux) { mux_end(); t_mux_chan = -1; } } } join_ssm{ssm_thread, muxed, tipp_done};      // every exit path waits for the second prover (it writes into `out` and `w`); an early exit of this thread releases its channel first
    if (e2) {
        if ((rc = e->sync())) return rc;                                   // w's vectors were filled on the main engine's stream
        if (muxed) { mux_begin(); t_mux_chan = 0; }
        ssm_thread = std::thread([&, e2]() {
            if (muxed) t_mux_chan = 1;
            if (hipSetDevice(e2->device) != hipSuccess) { ssm_rc = RIPP_ERR_DEVICE; ssm_err = "hipSetDevice failed on the second prover's thread"; }
            else { ssm_rc = ssm_block(e2); if (ssm_rc) ssm_err = g_err; }
            if (muxed) mux_done(1, ssm_rc); });
    }
    {   // tipa_proof_ab = TIPA::prove_with_srs_shift(srs, (a_r, b), (ck_1_r, ck_2), r)   (:138-143)
        G1A ha, hkb; G2A hb, hka;
        if ((rc = gipa_tipp_core(e, v, n, out->ab_com_steps, out->ab_transcript, ha, hb, hka, hkb, &r, sc))) return rc;
        if (trace_on()) fprintf(stderr, "[ripp] aggregate: TIPP GIPA rounds done at t=%.1f ms\n", now_ms() - t_start);
        G2J oa; G1J ob; Fr kc;
        if ((rc = tipp_kzg(e, srs, out->ab_transcript, rounds, r, hka, hkb, &oa, &ob, &kc, sc))) return rc;
        if (muxed) { mux_done(0, RIPP_OK); tipp_done = true; }
        const G1J ja = to_jac(ha), jkb = to_jac(hkb); const G2J jb = to_jac(hb), jka = to_jac(hka);
        std::memcpy(&out->ab_base_a, &ja, sizeof ja); std::memcpy(&out->ab_base_b, &jb, sizeof jb); std::memcpy(&out->ab_final_ck_a, &jka, sizeof jka); std::memcpy(&out->ab_final_ck_b, &jkb, sizeof jkb);
        std::memcpy(&out->ab_opening_a, &oa, sizeof oa); std::memcpy(&out->ab_opening_b, &ob, sizeof ob); std::memcpy(&out->ab_kzg_c, &kc, sizeof kc);
        if (trace_on()) fprintf(stderr, "[ripp] aggregate: TIPP KZG openings done at t=%.1f ms\n", now_ms() - t_start);
    }
    if (e2) {
        ssm_thread.join();
        if (ssm_rc) { set_err(ssm_err); return ssm_rc; }
        e2->collect_kernel_stats();
        e->stats.miller_products_ms += e2->stats.miller_products_ms; e->stats.fold_ms += e2->stats.fold_ms; e->stats.host_ms += e2->stats.host_ms;
        e->stats.kernel_miller_lines_ms_sum += e2->stats.kernel_miller_lines_ms_sum; e->stats.kernel_line_products_ms_sum += e2->stats.kernel_line_products_ms_sum;
        e->stats.kernel_miller_lines_launches += e2->stats.kernel_miller_lines_launches; e->stats.kernel_line_products_launches += e2->stats.kernel_line_products_launches;
        e->stats.pairs_lines += e2->stats.pairs_lines; e->stats.pairs_products += e2->stats.pairs_products;
    } else if ((rc = ssm_block(e))) return rc;
    return finish_stats(e, t_start, st, false);
}

API int32_t ripp_aggregate_proofs(const ripp_srs* srs, const ripp_g1a* a, const ripp_g2a* b, const ripp_g1a* c, size_t n, ripp_aggregate_proof* out, ripp_stats* st) {
    if (n < 2 || (n & (n - 1))) return RIPP_ERR_POW2;
    LOCK; ENGINE;
    if (!srs || !a || !b || !c || !out || !out->ab_com_steps || !out->ab_transcript || !out->c_com_gt || !out->c_com_g1 || !out->c_transcript) return RIPP_ERR_ARG;
    return aggregate_impl(e, srs, a, b, c, n, out, st, ShardCtx());
}
// aggregate_proofs across the communicator's ranks (config 5 on 8 GPUs): a, b, c = this rank's shard of the n_local * world proofs
// (local j <-> global j * world + rank); srs built for the GLOBAL n on every rank; every rank receives the full AggregateProof.
API int32_t ripp_aggregate_proofs_sharded(const ripp_srs* srs, const ripp_g1a* a, const ripp_g2a* b, const ripp_g1a* c, size_t n_local, ripp_aggregate_proof* out, ripp_stats* st) {
    if (n_local == 0 || (n_local & (n_local - 1))) return RIPP_ERR_POW2;
    LOCK; ENGINE;
    comm_mark_proof();
    if (!srs || !a || !b || !c || !out || !out->ab_com_steps || !out->ab_transcript || !out->c_com_gt || !out->c_com_g1 || !out->c_transcript) return RIPP_ERR_ARG;
    const ShardCtx sc = ShardCtx::from_comm();
    if (sc.world & (sc.world - 1)) { set_err("the number of ranks must be a power of two"); return RIPP_ERR_POW2; }
    if (n_local * (size_t)sc.world < 2) return RIPP_ERR_POW2;
    return aggregate_impl(e, srs, a, b, c, n_local, out, st, sc);
}

// ---- verifiers (gipa.rs:135-160, 322-415; tipa/mod.rs:242-301, 340-404; ssm.rs:270-331; groth16_aggregation.rs:162-231) -------
// Host: challenge replay and the O(log n) exponentiations of single GT / group elements (what the reference's verifier does
// serially).  Device: every pairing and the n-term MSMs.
extern "C++" {
// membership in the cyclotomic subgroup of Fp12* (x^(p^4 - p^2 + 1) == 1): every honest GT value is in it; the verifiers test the
// GT members of a proof before exponentiating them, because gt_pow_host is only an exponentiation there
static bool gt_in_cyclotomic(const Fp12& x) {
    const Fp2* c[6] = {&x.c0.c0, &x.c0.c1, &x.c0.c2, &x.c1.c0, &x.c1.c1, &x.c1.c2};
    bool zero = true; for (const Fp2* v : c) zero = zero && v->c0.is_zero() && v->c1.is_zero();
    return !zero && mul(frobenius(frobenius(x, 2), 2), x) == frobenius(x, 2);
}
// x^k for x in the cyclotomic subgroup: Granger-Scott squarings, NAF digits, and the inverse of x is its conjugate.
static Fp12 gt_pow_host(const Fp12& x, const Fr& k) {
    const Fr c = from_mont(k);
    int8_t d[260]; const int len = naf_recode(c.l, 8, d, 258);
    const Fp12 xi = conj(x);
    Fp12 acc = Fp12::one(); bool st = false;
    for (int i = len - 1; i >= 0; --i) {
        if (st) acc = cyclotomic_sqr(acc);
        if (d[i] != 0) { const Fp12& m = d[i] > 0 ? x : xi; acc = st ? mul(acc, m) : m; st = true; }
    }
    return acc;
}
template <class F> static Jac<F> smul_host(const Affine<F>& p, const Fr& k) { const Fr c = from_mont(k); return scalar_mul_bits(p, c.l, 255); }
template <class F> static Jac<F> load_jac(const void* p) { Jac<F> r; std::memcpy(&r, p, sizeof r); return r; }
static Fp12 load_gt(const ripp_gt* p) { Fp12 r; std::memcpy(&r, p, sizeof r); return r; }
static Fr load_fr(const ripp_fr* p) { Fr r; std::memcpy(&r, p, sizeof r); return r; }

// prod_i e(a_i, b_i) for a handful of host points
static int32_t pairing_host_pts(Engine* e, const std::vector<G1A>& a, const std::vector<G2A>& b, Fp12* out) {
    G1A* da; G2A* db; int32_t rc; ripp_gt z;
    if ((rc = upload<G1A>(e, e->tmpA, a.data(), a.size(), &da)) || (rc = upload<G2A>(e, e->tmpB, b.data(), b.size(), &db))) return rc;
    if ((rc = pairing_product_dev(e, da, db, a.size(), &z))) return rc;
    std::memcpy(out, &z, sizeof z); return RIPP_OK;
}
// e(a1, b1) == e(a2, b2)  as  e(a1, b1) * e(-a2, b2) == 1: one two-pair product, one final exponentiation
static int32_t pairing_eq(Engine* e, const G1J& a1, const G2J& b1, const G1J& a2, const G2J& b2, bool* ok) {
    Fp12 z; int32_t rc = pairing_host_pts(e, {to_affine(a1), neg(to_affine(a2))}, {to_affine(b1), to_affine(b2)}, &z); if (rc) return rc;
    *ok = (z == Fp12::one()); return RIPP_OK;
}
// polynomial_evaluation_product_form_from_transcript (tipa/mod.rs:393-404)
static Fr ck_poly_eval(const std::vector<Fr>& tr, const Fr& z, const Fr& r_shift) {
    Fr p = mul(mul(z, z), r_shift), acc = Fr::one();
    for (const Fr& x : tr) { acc = mul(acc, add(Fr::one(), mul(x, p))); p = mul(p, p); }
    return acc;
}
struct VSrs { G1J g, g_beta; G2J h, h_alpha; };
static VSrs load_vsrs(const ripp_verifier_srs* v) { return {load_jac<Fp>(&v->g), load_jac<Fp>(&v->g_beta), load_jac<Fp2>(&v->h), load_jac<Fp2>(&v->h_alpha)}; }
// verify_commitment_key_g2_kzg_opening (tipa/mod.rs:340-354): e(g, ck_final - h*eval) == e(g_beta - g*c, opening)
static int32_t kzg_verify_g2(Engine* e, const VSrs& v, const G2J& ck_final, const G2J& opening, const std::vector<Fr>& tr, const Fr& r_shift, const Fr& c, bool* ok) {
    const Fr ev = ck_poly_eval(tr, c, r_shift);
    const G2J l2 = add(ck_final, neg(smul_host(to_affine(v.h), ev)));
    const G1J r1 = add(v.g_beta, neg(smul_host(to_affine(v.g), c)));
    return pairing_eq(e, v.g, l2, r1, opening, ok);
}
// verify_commitment_key_g1_kzg_opening (tipa/mod.rs:356-370): e(ck_final - g*eval, h) == e(opening, h_alpha - h*c)
static int32_t kzg_verify_g1(Engine* e, const VSrs& v, const G1J& ck_final, const G1J& opening, const std::vector<Fr>& tr, const Fr& r_shift, const Fr& c, bool* ok) {
    const Fr ev = ck_poly_eval(tr, c, r_shift);
    const G1J l1 = add(ck_final, neg(smul_host(to_affine(v.g), ev)));
    const G2J r2 = add(v.h_alpha, neg(smul_host(to_affine(v.h), c)));
    return pairing_eq(e, l1, v.h, opening, r2, ok);
}
// ---- _compute_recursive_challenges (gipa.rs:322-363), one replay for every instantiation ----
// A commitment component is folded as  acc <- acc + c x_1 + c_inv x_2  (gipa.rs:358-360) in its own group: GT multiplicatively, G1 / G2 / Fr additively, the
// SSM placeholder not at all.  com_term is one k x, com_add the accumulation; a proof's points travel affine (their byte image is hashed), the sums Jacobian.
static Fp12 com_term(const Fp12& x, const Fr& k) { return gt_pow_host(x, k); }
template <class F> static Jac<F> com_term(const Affine<F>& x, const Fr& k) { return smul_host(x, k); }
static Fr com_term(const Fr& x, const Fr& k) { return mul(x, k); }
static fs::SSMPlaceholder com_term(fs::SSMPlaceholder x, const Fr&) { return x; }
static void com_add(Fp12& acc, const Fp12& t) { acc = mul(acc, t); }
template <class F> static void com_add(Jac<F>& acc, const Jac<F>& t) { acc = add(acc, t); }
static void com_add(Fr& acc, const Fr& t) { acc = add(acc, t); }
static void com_add(fs::SSMPlaceholder&, fs::SSMPlaceholder) {}
template <class X> using ComAcc = decltype(com_term(std::declval<const X&>(), std::declval<const Fr&>()));
// a term beside the calling thread: an exponentiation or scalar multiplication goes to the host pool, a field product is done at once.
// x and k are captured by reference: get() before they go out of scope.
template <class X> struct ComTermAsync {
    std::future<ComAcc<X>> f; ComAcc<X> v;
    ComTermAsync(const X& x, const Fr& k) {
        if constexpr (std::is_same<X, Fr>::value || std::is_same<X, fs::SSMPlaceholder>::value) v = com_term(x, k);
        else f = host_pool().submit([&x, &k]() { return com_term(x, k); });
    }
    ComAcc<X> get() { return f.valid() ? f.get() : v; }
};
static bool com_member_ok(const Fp12& x) { return gt_in_cyclotomic(x); }      // not a GT element: reject (gt_pow_host is only an exponentiation in the cyclotomic subgroup)
template <class X> static bool com_member_ok(const X&) { return true; }
// Folds the steps of `rounds` rounds into (al, ar, at) = (com_a, com_b, com_t) and writes the challenges to tr in ROUND order.  load(k, com_1, com_2) fills round
// k's members.  false: a GT member is not in the cyclotomic subgroup (found before anything of that round is exponentiated).  Of a round's up to six
// exponentiations / scalar multiplications the first (c com_1.l: costly in every instantiation) runs here, the others on pool threads.
template <class L, class R, class T, class Load> static bool gipa_replay(ComAcc<L>& al, ComAcc<R>& ar, ComAcc<T>& at, size_t rounds, std::vector<Fr>& tr, Load&& load) {
    tr.resize(rounds);
    for (size_t k = 0; k < rounds; ++k) {
        fs::Com<L, R, T> s1, s2; load(k, s1, s2);
        for (const fs::Com<L, R, T>* s : {&s1, &s2}) if (!com_member_ok(s->l) || !com_member_ok(s->r) || !com_member_ok(s->t)) return false;
        Fr c_inv; const Fr c = fs::gipa_challenge(k ? &tr[k - 1] : nullptr, s1, s2, c_inv);
        ComTermAsync<L> l2(s2.l, c_inv); ComTermAsync<R> r1(s1.r, c), r2(s2.r, c_inv); ComTermAsync<T> t1(s1.t, c), t2(s2.t, c_inv);
        const ComAcc<L> l1 = com_term(s1.l, c);
        com_add(al, l1); com_add(al, l2.get()); com_add(ar, r1.get()); com_add(ar, r2.get()); com_add(at, t1.get()); com_add(at, t2.get());
        tr[k] = c;
    }
    return true;
}
static G1A load_g1a(const ripp_g1j* p) { return to_affine(load_jac<Fp>(p)); }
static G2A load_g2a(const ripp_g2j* p) { return to_affine(load_jac<Fp2>(p)); }
// TIPP: com_steps[k] = com_1.{0,1,2}, com_2.{0,1,2}
static bool tipp_replay(const ripp_gt com[3], const ripp_gt* com_steps, size_t rounds, std::vector<Fr>& tr, Fp12 out[3]) {
    for (int j = 0; j < 3; ++j) out[j] = load_gt(&com[j]);
    return gipa_replay<Fp12, Fp12, Fp12>(out[0], out[1], out[2], rounds, tr, [&](size_t k, auto& s1, auto& s2) { std::memcpy(&s1, &com_steps[6 * k], sizeof s1); std::memcpy(&s2, &com_steps[6 * k + 3], sizeof s2); });
}
// the second-tier GIPAWithSSM instantiation (MultiexponentiationInnerProduct<G1>, AFGHO commitment): folds the steps into (ca, ct) = (com_a, com_t)
static bool ssm_replay(Fp12& ca, G1J& ct, const ripp_gt* com_gt, const ripp_g1j* com_g1, size_t rounds, std::vector<Fr>& tr) {
    fs::SSMPlaceholder cb;
    return gipa_replay<Fp12, fs::SSMPlaceholder, G1A>(ca, cb, ct, rounds, tr, [&](size_t k, auto& s1, auto& s2) {
        s1 = {load_gt(&com_gt[2 * k]), {}, load_g1a(&com_g1[2 * k])}; s2 = {load_gt(&com_gt[2 * k + 1]), {}, load_g1a(&com_g1[2 * k + 1])}; });
}
// exponents of _compute_final_commitment_keys (gipa.rs:365-399) by doubling over the reversed transcript (tr in ROUND order): powers of c^-1 for ck_a, of c for ck_b
static std::vector<Fr> final_key_exponents(const std::vector<Fr>& tr, bool inverse) {
    const size_t rounds = tr.size();
    std::vector<Fr> ex((size_t)1 << rounds); ex[0] = Fr::one(); size_t cnt = 1;
    for (size_t i = 0; i < rounds; ++i) {
        const Fr c = inverse ? inv(tr[rounds - 1 - i]) : tr[rounds - 1 - i];
        for (size_t j = 0; j < ((size_t)1 << i); ++j) ex[cnt + j] = mul(ex[j], c);
        cnt += (size_t)1 << i;
    }
    return ex;
}
// b_base of the structured scalar vector (1, b, b^2, ..) (ssm.rs:108-114, 315-321); tr in ROUND order
static Fr ssm_b_base(const std::vector<Fr>& tr, const Fr& scalar_b) {
    Fr p2b = scalar_b, bb = Fr::one();
    for (size_t i = 0; i < tr.size(); ++i) { bb = mul(bb, add(Fr::one(), mul(inv(tr[tr.size() - 1 - i]), p2b))); p2b = mul(p2b, p2b); }
    return bb;
}
// What TIPA::verify_with_srs_shift does between the replay and the base check, for every instantiation (tipa/mod.rs:252-289): the KZG challenge from the last
// round's challenge and both final keys, the opening check of ck_a (inverse transcript, shift r_shift^-1) and of ck_b.  trf: the replayed transcript in ROUND
// order.  *ok = both openings hold; kaa, kba: the affine final keys, which the caller's base check needs.
static int32_t tipa_verify_tail(Engine* e, const ripp_verifier_srs* v_srs, const std::vector<Fr>& trf, const ripp_g2j* final_ck_a, const ripp_g1j* final_ck_b,
                                const ripp_g2j* opening_a, const ripp_g1j* opening_b, const ripp_fr* r_shift, G2A& kaa, G1A& kba, bool* ok) {
    const VSrs v = load_vsrs(v_srs); const size_t rounds = trf.size();
    std::vector<Fr> tr(rounds), tri(rounds); for (size_t i = 0; i < rounds; ++i) { tr[i] = trf[rounds - 1 - i]; tri[i] = inv(tr[i]); }
    const G2J ka = load_jac<Fp2>(final_ck_a), oa = load_jac<Fp2>(opening_a); const G1J kb = load_jac<Fp>(final_ck_b), ob = load_jac<Fp>(opening_b);
    kaa = to_affine(ka); kba = to_affine(kb);
    const Fr c = fs::kzg_challenge(tr[0], kaa, &kba);                                                                    // :257-272
    bool ok_a = false, ok_b = false; int32_t rc;
    if ((rc = kzg_verify_g2(e, v, ka, oa, tri, inv(load_fr(r_shift)), c, &ok_a))) return rc;                             // :274-281
    if ((rc = kzg_verify_g1(e, v, kb, ob, tr, Fr::one(), c, &ok_b))) return rc;                                          // :282-289
    *ok = ok_a && ok_b; return RIPP_OK;
}
}  // extern "C++"

API int32_t ripp_gipa_tipp_verify(const ripp_g2j* ck_a, const ripp_g1j* ck_b, size_t n, const ripp_gt com[3], const ripp_gt* com_steps, size_t rounds,
                                  const ripp_g1j* base_a, const ripp_g2j* base_b, int32_t* accept) {
    if (n == 0 || (n & (n - 1))) return RIPP_ERR_POW2;
    if (!ck_a || !ck_b || !com || !base_a || !base_b || !accept || (rounds && !com_steps) || ((size_t)1 << rounds) != n) return RIPP_ERR_ARG;
    std::vector<Fr> tr; Fp12 bc[3];
    if (!tipp_replay(com, com_steps, rounds, tr, bc)) { *accept = 0; return RIPP_OK; }
    const std::vector<Fr> ea = final_key_exponents(tr, true), eb = final_key_exponents(tr, false);      // then one MSM per key
    ripp_g2j ka; ripp_g1j kb; int32_t rc;
    if ((rc = ripp_msm_g2_j(ck_a, n, reinterpret_cast<const ripp_fr*>(ea.data()), n, &ka))) return rc;
    if ((rc = ripp_msm_g1_j(ck_b, n, reinterpret_cast<const ripp_fr*>(eb.data()), n, &kb))) return rc;
    LOCK; ENGINE;
    const G1A a = to_affine(load_jac<Fp>(base_a)), kba = to_affine(load_jac<Fp>(&kb)); const G2A b = to_affine(load_jac<Fp2>(base_b)), kaa = to_affine(load_jac<Fp2>(&ka));
    Fp12 e1, e2, e3;                                                          // _verify_base_commitment (gipa.rs:401-415)
    if ((rc = pairing_host_pts(e, {a}, {kaa}, &e1)) || (rc = pairing_host_pts(e, {kba}, {b}, &e2)) || (rc = pairing_host_pts(e, {a}, {b}, &e3))) return rc;
    *accept = (e1 == bc[0] && e2 == bc[1] && e3 == bc[2]) ? 1 : 0;
    return RIPP_OK;
}

API int32_t ripp_tipa_tipp_verify(const ripp_verifier_srs* v_srs, const ripp_gt com[3], const ripp_gt* com_steps, size_t rounds,
                                  const ripp_g1j* base_a, const ripp_g2j* base_b, const ripp_g2j* final_ck_a, const ripp_g1j* final_ck_b,
                                  const ripp_g2j* opening_a, const ripp_g1j* opening_b, const ripp_fr* r_shift, int32_t* accept) {
    if (!v_srs || !com || !com_steps || !base_a || !base_b || !final_ck_a || !final_ck_b || !opening_a || !opening_b || !r_shift || !accept || rounds == 0) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    std::vector<Fr> trf; Fp12 bc[3];
    if (!tipp_replay(com, com_steps, rounds, trf, bc)) { *accept = 0; return RIPP_OK; }                                  // :249-251
    G2A kaa; G1A kba; bool ok = false; int32_t rc;
    if ((rc = tipa_verify_tail(e, v_srs, trf, final_ck_a, final_ck_b, opening_a, opening_b, r_shift, kaa, kba, &ok))) return rc;
    const G1A a = load_g1a(base_a); const G2A b = load_g2a(base_b);
    Fp12 e1, e2, e3;                                                                                                     // :292-298
    if ((rc = pairing_host_pts(e, {a}, {kaa}, &e1)) || (rc = pairing_host_pts(e, {kba}, {b}, &e2)) || (rc = pairing_host_pts(e, {a}, {b}, &e3))) return rc;
    *accept = (ok && e1 == bc[0] && e2 == bc[1] && e3 == bc[2]) ? 1 : 0;
    return RIPP_OK;
}

// TIPAWithSSM::verify_with_structured_scalar_message (ssm.rs:270-331), engine in hand and the lock held by the caller (ripp_pc_verify runs it beside its KZG check):
// replay, KZG check of the final key, base check
static int32_t tipa_ssm_verify_core(Engine* e, const ripp_verifier_srs* v_srs, const ripp_gt* com_a, const ripp_g1j* com_t, const ripp_fr* scalar_b,
                                    const ripp_gt* com_gt, const ripp_g1j* com_g1, size_t rounds, const ripp_g1j* base_a,
                                    const ripp_g2j* final_ck_a, const ripp_g2j* opening_a, int32_t* accept) {
    const VSrs v = load_vsrs(v_srs);
    Fp12 ca = load_gt(com_a); G1J ct = load_jac<Fp>(com_t);
    std::vector<Fr> trf;
    if (!ssm_replay(ca, ct, com_gt, com_g1, rounds, trf)) { *accept = 0; return RIPP_OK; }
    std::vector<Fr> tri(rounds); for (size_t i = 0; i < rounds; ++i) tri[i] = inv(trf[rounds - 1 - i]);
    const G2J ka = load_jac<Fp2>(final_ck_a), oa = load_jac<Fp2>(opening_a); const G2A kaa = to_affine(ka);
    const Fr c = fs::kzg_challenge(trf[rounds - 1], kaa, nullptr);                                                       // ssm.rs:289-303
    bool ok_a = false; int32_t rc;
    if ((rc = kzg_verify_g2(e, v, ka, oa, tri, Fr::one(), c, &ok_a))) return rc;                                         // ssm.rs:305-312
    const G1A a = to_affine(load_jac<Fp>(base_a));
    Fp12 e1; if ((rc = pairing_host_pts(e, {a}, {kaa}, &e1))) return rc;                                                 // ssm.rs:324-328
    *accept = (ok_a && e1 == ca && eq(smul_host(a, ssm_b_base(trf, load_fr(scalar_b))), ct)) ? 1 : 0;                // ssm.rs:315-321
    return RIPP_OK;
}

API int32_t ripp_tipa_ssm_verify(const ripp_verifier_srs* v_srs, const ripp_gt* com_a, const ripp_g1j* com_t, const ripp_fr* scalar_b,
                                 const ripp_gt* com_gt, const ripp_g1j* com_g1, size_t rounds, const ripp_g1j* base_a,
                                 const ripp_g2j* final_ck_a, const ripp_g2j* opening_a, int32_t* accept) {
    if (!v_srs || !com_a || !com_t || !scalar_b || !com_gt || !com_g1 || !base_a || !final_ck_a || !opening_a || !accept || rounds == 0) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    return tipa_ssm_verify_core(e, v_srs, com_a, com_t, scalar_b, com_gt, com_g1, rounds, base_a, final_ck_a, opening_a, accept);
}

API int32_t ripp_verify_aggregate_proof(const ripp_verifier_srs* v_srs, const ripp_groth16_vk* vk, const ripp_fr* public_inputs, size_t n, size_t m,
                                        const ripp_aggregate_proof* pf, int32_t* accept) {
    if (n < 2 || (n & (n - 1))) return RIPP_ERR_POW2;
    if (!v_srs || !vk || !vk->gamma_abc_g1 || (m && !public_inputs) || !pf || !accept) return RIPP_ERR_ARG;
    if (vk->gamma_abc_len != m + 1) { set_err("assert_eq!(vk.gamma_abc_g1.len(), public_inputs[0].len() + 1) (groth16_aggregation.rs:214)"); return RIPP_ERR_ARG; }
    const size_t rounds = log2_sz(n);
    const Fr r = fs::aggregation_challenge(load_gt(&pf->com_a), load_gt(&pf->com_b), load_gt(&pf->com_c));             // :172-184
    int32_t ok_ab = 0, ok_c = 0, rc;
    const ripp_gt com_ab[3] = {pf->com_a, pf->com_b, pf->ip_ab};
    if ((rc = ripp_tipa_tipp_verify(v_srs, com_ab, pf->ab_com_steps, rounds, &pf->ab_base_a, &pf->ab_base_b, &pf->ab_final_ck_a, &pf->ab_final_ck_b,   // :187-198
                                    &pf->ab_opening_a, &pf->ab_opening_b, reinterpret_cast<const ripp_fr*>(&r), &ok_ab))) return rc;
    if ((rc = ripp_tipa_ssm_verify(v_srs, &pf->com_c, &pf->agg_c, reinterpret_cast<const ripp_fr*>(&r), pf->c_com_gt, pf->c_com_g1, rounds, &pf->c_base_a,   // :199-205
                                   &pf->c_final_ck_a, &pf->c_opening_a, &ok_c))) return rc;
    LOCK; ENGINE;
    // r_sum = (r^n - 1) / (r - 1)   (:209-210)
    Fr rn = Fr::one(); std::vector<Fr> rv(n); for (size_t i = 0; i < n; ++i) { rv[i] = rn; rn = mul(rn, r); }
    const Fr r_sum = mul(sub(rn, Fr::one()), inv(sub(r, Fr::one())));
    G1A alpha; G2A beta, gamma, delta; std::memcpy(&alpha, &vk->alpha_g1, sizeof alpha); std::memcpy(&beta, &vk->beta_g2, sizeof beta);
    std::memcpy(&gamma, &vk->gamma_g2, sizeof gamma); std::memcpy(&delta, &vk->delta_g2, sizeof delta);
    const G1A* abc = reinterpret_cast<const G1A*>(vk->gamma_abc_g1);
    G1J g_ic = smul_host(abc[0], r_sum);                                                                                 // :215-226
    const Fr* pub = reinterpret_cast<const Fr*>(public_inputs);
    for (size_t i = 0; i < m; ++i) {
        Fr ip = Fr::zero(); for (size_t k = 0; k < n; ++k) ip = add(ip, mul(pub[k * m + i], rv[k]));                     // ScalarInnerProduct(inputs[:, i], r_vec)
        g_ic = add(g_ic, smul_host(abc[i + 1], ip));
    }
    // ip_ab == e(alpha * r_sum, beta) + e(g_ic, gamma) + e(agg_c, delta)   (:211, 227-229): one three-pair product
    Fp12 rhs;
    if ((rc = pairing_host_pts(e, {to_affine(smul_host(alpha, r_sum)), to_affine(g_ic), to_affine(load_jac<Fp>(&pf->agg_c))}, {beta, gamma, delta}, &rhs))) return rc;
    *accept = (ok_ab && ok_c && load_gt(&pf->ip_ab) == rhs) ? 1 : 0;
    return RIPP_OK;
}

