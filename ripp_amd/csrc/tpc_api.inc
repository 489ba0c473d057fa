// Included by engine.hip inside its `extern "C"` block (after poly_commit_api.inc: it builds on its two-tier core and matrix uploads).
// ---- transparent polynomial commitments: ip_proofs/src/applications/poly_commit/transparent.rs on the device -------------------------------
// BivariatePolynomialCommitment (:86-212) and UnivariatePolynomialCommitment (:214-330) behind a resident commitment-key handle, and the two
// GIPAWithSSM arguments they are made of (tipa/structured_scalar_message.rs:56-128):
//   second tier  GIPAWithSSM<MultiexponentiationInnerProduct<G1>, AFGHOCommitmentG1, IdentityCommitment<G1>>   the rounds of tipa_ssm_core (tipa_ssm_rounds)
//   first tier   GIPAWithSSM<ScalarInnerProduct, PedersenCommitment<G1>, IdentityCommitment<Fr>>                the kernels of tpc.hpp
// commit, the head of open and the loading of the second tier are the two-tier core of poly_commit_api.inc on this handle's keys; open keeps y_eval_coeffs on
// the device from the partial evaluation through the last first-tier fold; the verifiers replay the transcripts on the host (the second tier's with the
// TIPAWithSSM verifier's ssm_replay, tipa_api.inc) and run the two final-key MSMs on the resident keys.
// Every entry point takes LOCK once and calls the unlocked cores; none calls an exported function.

extern "C++" {
static bool tpc_degrees_ok(size_t x_degree, size_t y_degree) { return x_degree < ((size_t)1 << 24) && y_degree < ((size_t)1 << 28) && x_degree && y_degree && is_pow2(x_degree + 1) && is_pow2(y_degree + 1); }
static std::vector<double> g_tpc_round_ms;      // commitment + inner-product phase of every round of the last first-tier prover (ripp_tpc_round_ms)
}  // extern "C++"

// UnivariatePolynomialCommitment::bivariate_degrees (transparent.rs:221-227); host only, needs no device
API int32_t ripp_tpc_univariate_degrees(size_t degree, size_t* x_degree, size_t* y_degree) { return sqrt_split(degree, 4, "ripp_tpc_univariate_degrees", "transparent.rs:223-226", x_degree, y_degree); }

// first_tier_ck (y_degree + 1 G1 points, affine, with the extended GLV form the batched MSM gathers from) and second_tier_ck (x_degree + 1 G2 points)
struct ripp_tpc_ck { DevBuf k1, ext, k2; size_t nx = 0, ny = 0; };

extern "C++" {
static TwoTier tpc_key(const ripp_tpc_ck* s) { return {static_cast<const G1A*>(s->k1.p), static_cast<QAff<Fp>*>(s->ext.p), static_cast<const G2A*>(s->k2.p), s->nx, s->ny}; }
static void tpc_ck_free(ripp_tpc_ck* s) { s->k1.release(); s->ext.release(); s->k2.release(); delete s; }
static int32_t tpc_ck_alloc(size_t x_degree, size_t y_degree, ripp_tpc_ck** out) {
    ripp_tpc_ck* s = new ripp_tpc_ck(); s->nx = x_degree + 1; s->ny = y_degree + 1; int32_t rc;
    if ((rc = s->k1.reserve(s->ny * sizeof(G1A))) || (rc = s->ext.reserve(2 * s->ny * sizeof(G1A))) || (rc = s->k2.reserve(s->nx * sizeof(G2A)))) { tpc_ck_free(s); return rc; }
    *out = s; return RIPP_OK;
}
// the extended form once k1 is in place
static int32_t tpc_ck_finish(Engine* e, ripp_tpc_ck* s) { int32_t rc = two_tier_extend(e, tpc_key(s)); return rc ? rc : e->sync(); }
// out[i] = (seed + i) * generator, normalised: the points of ripp_synth_g1 / ripp_synth_g2 (start = seed, first = 0, stride = 1)
template <class F> static int32_t tpc_synth_dev(Engine* e, const Affine<F>& g, uint64_t seed, size_t n, Affine<F>* out) {
    DevBuf& jac = std::is_same<F, Fp>::value ? e->jacG1 : e->jacG2;
    int32_t rc; if ((rc = jac.reserve(n * sizeof(Jac<F>)))) return rc;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_synth_points<F>), dim3(nblk(n, 64)), dim3(64), 0, e->stream, g, seed, (uint64_t)0, (uint64_t)1, (uint32_t)n, jac.as<Jac<F>>());
    HIPCHK(hipGetLastError());
    return e->normalize_dev<F>(jac.as<Jac<F>>(), n, out);
}
}  // extern "C++"

// BivariatePolynomialCommitment::setup (transparent.rs:89-99) with the generators' seeds given instead of an RNG: key i = (seed + i) * generator, on the device
API int32_t ripp_tpc_ck_setup(uint64_t seed_g1, uint64_t seed_g2, size_t x_degree, size_t y_degree, ripp_tpc_ck** out) {
    if (!out) return RIPP_ERR_ARG;
    if (!tpc_degrees_ok(x_degree, y_degree)) { set_err("ripp_tpc_ck_setup: x_degree + 1 and y_degree + 1 must be powers of two >= 2 (both tiers halve their keys)"); return RIPP_ERR_POW2; }
    LOCK; ENGINE;
    ripp_tpc_ck* s; int32_t rc = tpc_ck_alloc(x_degree, y_degree, &s); if (rc) return rc;
    if ((rc = tpc_synth_dev<Fp>(e, g1_generator(), seed_g1, s->ny, s->k1.as<G1A>())) || (rc = tpc_synth_dev<Fp2>(e, g2_generator(), seed_g2, s->nx, s->k2.as<G2A>())) ||
        (rc = tpc_ck_finish(e, s))) { tpc_ck_free(s); return rc; }
    ++g_live_handles; *out = s; return RIPP_OK;
}
// the same from caller-supplied keys: first_tier_ck[y_degree + 1], second_tier_ck[x_degree + 1], both affine
API int32_t ripp_tpc_ck_create(const ripp_g1a* first_tier_ck, size_t y_degree, const ripp_g2a* second_tier_ck, size_t x_degree, ripp_tpc_ck** out) {
    if (!first_tier_ck || !second_tier_ck || !out) return RIPP_ERR_ARG;
    if (!tpc_degrees_ok(x_degree, y_degree)) { set_err("ripp_tpc_ck_create: x_degree + 1 and y_degree + 1 must be powers of two >= 2 (both tiers halve their keys)"); return RIPP_ERR_POW2; }
    LOCK; ENGINE;
    ripp_tpc_ck* s; int32_t rc = tpc_ck_alloc(x_degree, y_degree, &s); if (rc) return rc;
    if (hipMemcpyAsync(s->k1.p, first_tier_ck, s->ny * sizeof(G1A), hipMemcpyHostToDevice, e->stream) != hipSuccess ||
        hipMemcpyAsync(s->k2.p, second_tier_ck, s->nx * sizeof(G2A), hipMemcpyHostToDevice, e->stream) != hipSuccess) { tpc_ck_free(s); set_err("ripp_tpc_ck_create: hipMemcpyAsync failed"); return RIPP_ERR_DEVICE; }
    if ((rc = tpc_ck_finish(e, s))) { tpc_ck_free(s); return rc; }
    ++g_live_handles; *out = s; return RIPP_OK;
}
API void ripp_tpc_ck_destroy(ripp_tpc_ck* s) { if (!s) return; LOCK; tpc_ck_free(s); --g_live_handles; }
// parse_bivariate_degrees_from_ck (transparent.rs:229-233)
API int32_t ripp_tpc_ck_degrees(const ripp_tpc_ck* s, size_t* x_degree, size_t* y_degree) {
    if (!s || !x_degree || !y_degree) return RIPP_ERR_ARG;
    *x_degree = s->nx - 1; *y_degree = s->ny - 1; return RIPP_OK;
}
API int32_t ripp_tpc_ck_keys(const ripp_tpc_ck* s, ripp_g1a* first_tier_ck, ripp_g2a* second_tier_ck) {
    if (!s || !first_tier_ck || !second_tier_ck) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    HIPCHK(hipMemcpyAsync(first_tier_ck, s->k1.p, s->ny * sizeof(G1A), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(second_tier_ck, s->k2.p, s->nx * sizeof(G2A), hipMemcpyDeviceToHost, e->stream));
    return e->sync();
}
// diagnostics: milliseconds from the launch of a round's commitments and inner products to their arrival on the host, for every round (key lengths
// n, n / 2, .. 2) of the LAST first-tier prover of this process; returns the number of rounds (tools/tpc_first_tier_ab.py)
API int32_t ripp_tpc_round_ms(double* out, size_t cap) {
    LOCK;
    for (size_t i = 0; out && i < cap && i < g_tpc_round_ms.size(); ++i) out[i] = g_tpc_round_ms[i];
    return (int32_t)g_tpc_round_ms.size();
}

extern "C++" {
static int32_t tpc_reserve_first(Engine* e, size_t n) {
    int32_t rc;
    for (DevBuf* b : {&e->tpc_m, &e->tpc_m2, &e->tpc_b, &e->tpc_b2}) if ((rc = b->reserve(n * sizeof(Fr)))) return rc;
    for (DevBuf* b : {&e->tpc_k, &e->tpc_k2}) if ((rc = b->reserve(n * sizeof(G1A)))) return rc;
    if ((rc = e->tpc_out.reserve(2 * sizeof(G1J))) || (rc = e->tpc_part.reserve(2 * 1024 * sizeof(Fr)))) return rc;
    return RIPP_OK;
}

// Both inner products of a scalar round, <a[h:], b[:h]> and <a[:h], b[h:]>: launch() enqueues k_fr_dot2 on the engine's stream (one partial per block and product
// into dpart, 2 * 1024 Fr) and the copy of the partials behind it; sum() adds them up once that stream has been synchronised.
struct FrDot2 {
    std::vector<Fr> part = std::vector<Fr>(2 * 1024); unsigned blocks = 0;
    int32_t launch(Engine* e, const Fr* a, const Fr* b, size_t h, DevBuf& dpart) {
        blocks = std::min<unsigned>(1024, nblk(h, 256));
        hipLaunchKernelGGL(k_fr_dot2, dim3(blocks, 2), dim3(256), 0, e->stream, a, b, (uint32_t)h, dpart.as<Fr>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(part.data(), dpart.p, 2 * blocks * sizeof(Fr), hipMemcpyDeviceToHost, e->stream));
        return RIPP_OK;
    }
    void sum(Fr ip[2]) const {
        ip[0] = ip[1] = Fr::zero();
        for (unsigned k = 0; k < blocks; ++k) { ip[0] = add(ip[0], part[k]); ip[1] = add(ip[1], part[blocks + k]); }
    }
};

// GIPA<ScalarInnerProduct, PedersenCommitment<G1>, SSMPlaceholder, IdentityCommitment<Fr>>::_prove (gipa.rs:181-312) on e->tpc_m (message), e->tpc_b
// (structured scalars) and e->tpc_k (keys), n elements each, filled on e->stream by the caller (tpc_reserve_first).  ext0 (optional): the extended form
// of the n keys as they stand before the first round (a resident ripp_tpc_ck has it); after every key fold the batch pipeline rebuilds its own.
// com_g1[r][2] = (com_1.0, com_2.0), com_fr[r][2] = (com_1.2[0], com_2.2[0]), transcript[r]: ROUND order.
// A round's two Pedersen commitments are ONE crossed pass of the batched MSM pipeline (tpc.hpp) from key length e->cfg.tpc_cross_min on; below it, and under
// the legacy MSM switches, two single MSMs on two streams.
static int32_t tpc_scalar_rounds(Engine* e, size_t n, const QAff<Fp>* ext0, ripp_g1j* com_g1, ripp_fr* com_fr, ripp_fr* transcript, Fr& ha, Fr& hb) {
    int32_t rc; if ((rc = e->sync())) return rc;
    size_t len = n, round = 0; Fr prev_c = Fr::zero();
    g_tpc_round_ms.clear();
    FrDot2 dot;
    while (len > 1) {
        const size_t h = len / 2;
        const Fr* M = e->tpc_m.as<Fr>(); const Fr* B = e->tpc_b.as<Fr>(); const G1A* K = e->tpc_k.as<G1A>();
        const bool cross = !e->msm_batch_legacy() && len >= e->cfg.tpc_cross_min;
        const double tp = now_ms();
        G1J cm[2];
        if (cross) {         // com_1.0 = <ck[:h], m[h:]>, com_2.0 = <ck[h:], m[:h]> as rows 0 and 1 over the whole key vector   gipa.rs:209-231
            if ((rc = e->msm_batch_dev<Fp>(K, round == 0 ? ext0 : nullptr, M, 2, len, 0, e->tpc_out.as<G1J>(), (uint32_t)h))) return rc;
            HIPCHK(hipMemcpyAsync(cm, e->tpc_out.p, sizeof cm, hipMemcpyDeviceToHost, e->stream));
        } else {
            if ((rc = e->msm_launch<Fp>(e->msm_scratch[0], e->stream2, K, M + h, h)) || (rc = e->msm_launch<Fp>(e->msm_scratch[1], e->stream3, K + h, M, h))) return rc;
        }
        if ((rc = dot.launch(e, M, B, h, e->tpc_part)) || (rc = e->sync())) return rc;                                       // <m[h:], b[:h]>, <m[:h], b[h:]>
        if (!cross) {
            HIPCHK(hipStreamSynchronize(e->stream2)); HIPCHK(hipStreamSynchronize(e->stream3));
            cm[0] = *reinterpret_cast<const G1J*>(e->msm_scratch[0].host_out); cm[1] = *reinterpret_cast<const G1J*>(e->msm_scratch[1].host_out);
        }
        g_tpc_round_ms.push_back(now_ms() - tp);
        if ((rc = fold_precompute<Fp>(e, e->stream2, K + h, h, g_tpc_pre))) return rc;        // small rounds: during the host phase
        const double th = now_ms();                                                        // (no Miller loop in this tier: stats.miller_products_ms stays 0, the commitments are total_ms less fold_ms and host_ms)
        Fr ip[2]; dot.sum(ip);
        Fr c_inv; const Fr c = fs::gipa_challenge(round ? &prev_c : nullptr, fs::Com{to_affine(cm[0]), fs::SSMPlaceholder{}, ip[0]}, fs::Com{to_affine(cm[1]), fs::SSMPlaceholder{}, ip[1]}, c_inv);
        e->stats.host_ms += now_ms() - th;
        std::memcpy(&com_g1[2 * round], cm, sizeof cm); std::memcpy(&com_fr[2 * round], ip, sizeof ip); std::memcpy(&transcript[round], &c, sizeof c);
        prev_c = c;
        const double tf = now_ms();
        rc = fork_join_folds(e, [&]() -> int32_t {
            int32_t r2;
            if ((r2 = fold_dev<Fp>(e, e->stream2, K + h, K, h, c_inv, e->tpc_jac, e->qtab, e->tpc_k2.as<G1A>(), &g_tpc_pre))) return r2;       // ck <- ck_2 * c_inv + ck_1
            hipLaunchKernelGGL(k_fold_fr2, dim3(nblk(h, 256), 2), dim3(256), 0, e->stream3, M, B, (uint32_t)h, c, c_inv, e->tpc_m2.as<Fr>(), e->tpc_b2.as<Fr>());   // m <- m_1 * c + m_2, b <- b_2 * c_inv + b_1
            HIPCHK(hipGetLastError());
            return RIPP_OK;
        });
        if (rc) return rc;
        e->stats.fold_ms += now_ms() - tf;
        std::swap(e->tpc_m, e->tpc_m2); std::swap(e->tpc_b, e->tpc_b2); std::swap(e->tpc_k, e->tpc_k2);
        len = h; ++round;
    }
    HIPCHK(hipMemcpy(&ha, e->tpc_m.p, sizeof ha, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(&hb, e->tpc_b.p, sizeof hb, hipMemcpyDeviceToHost));
    return RIPP_OK;
}

// sum_i ea[i] * keys[i] over device-resident keys
template <class F> static int32_t tpc_final_key(Engine* e, const Affine<F>* dkeys, const std::vector<Fr>& ea, Jac<F>* out) {
    Fr* ds; int32_t rc;
    if ((rc = upload<Fr>(e, e->tmpR, ea.data(), ea.size(), &ds))) return rc;
    return e->msm_dev<F>(dkeys, ds, ea.size(), out);                                  // synchronises: ea outlives the copy
}

// GIPAWithSSM::verify_with_structured_scalar_message (structured_scalar_message.rs:86-127), first-tier instantiation; dkeys: n = 2^rounds G1 keys on the device.
// com = (com_a: the Pedersen commitment, com_t: the inner product).
static int32_t tpc_scalar_verify_core(Engine* e, const G1A* dkeys, size_t rounds, const G1J& com_a, const Fr& com_t, const Fr& scalar_b,
                                      const ripp_g1j* com_g1, const ripp_fr* com_fr, const Fr& base_a, const Fr& base_b, bool* ok) {
    G1J ca = com_a; Fr ct = com_t; fs::SSMPlaceholder cb;
    std::vector<Fr> tr;
    gipa_replay<G1A, fs::SSMPlaceholder, Fr>(ca, cb, ct, rounds, tr, [&](size_t k, auto& s1, auto& s2) {                 // gipa.rs:329-360 (no GT member: nothing to reject)
        s1 = {load_g1a(&com_g1[2 * k]), {}, load_fr(&com_fr[2 * k])}; s2 = {load_g1a(&com_g1[2 * k + 1]), {}, load_fr(&com_fr[2 * k + 1])}; });
    G1J ka; int32_t rc;
    if ((rc = tpc_final_key<Fp>(e, dkeys, final_key_exponents(tr, true), &ka))) return rc;
    // gipa_valid (:100-106, gipa.rs:401-415): the Pedersen commitment of a_base under the final key, the (empty) placeholder commitment, the product with the
    // proof's own r_base.1; base_valid (:108-125): the same with b_base recomputed from scalar_b
    const bool com_ok = eq(smul_host(to_affine(ka), base_a), ca);
    const bool gipa_valid = com_ok && mul(base_a, base_b) == ct;
    const bool base_valid = com_ok && mul(base_a, ssm_b_base(tr, scalar_b)) == ct;
    *ok = gipa_valid && base_valid; return RIPP_OK;
}
// the same for the second tier; dkeys: n = 2^rounds G2 keys on the device.  com = (com_a in GT, com_t in G1).  Replay, final-key MSM, base checks.
static int32_t tpc_mexp_verify_core(Engine* e, const G2A* dkeys, size_t rounds, const Fp12& com_a, const G1J& com_t, const Fr& scalar_b,
                                    const ripp_gt* com_gt, const ripp_g1j* com_g1, const G1J& base_a, const Fr& base_b, bool* ok) {
    Fp12 ca = com_a; G1J ct = com_t; std::vector<Fr> tr;
    if (!ssm_replay(ca, ct, com_gt, com_g1, rounds, tr)) { *ok = false; return RIPP_OK; }
    G2J ka; int32_t rc;
    if ((rc = tpc_final_key<Fp2>(e, dkeys, final_key_exponents(tr, true), &ka))) return rc;
    const G1A a = to_affine(base_a);
    Fp12 e1; if ((rc = pairing_host_pts(e, {a}, {to_affine(ka)}, &e1))) return rc;
    const bool com_ok = e1 == ca;
    const bool gipa_valid = com_ok && eq(smul_host(a, base_b), ct);
    const bool base_valid = com_ok && eq(smul_host(a, ssm_b_base(tr, scalar_b)), ct);
    *ok = gipa_valid && base_valid; return RIPP_OK;
}

static bool tpc_opening_ok(const ripp_tpc_opening* o) { return o && o->s_com_gt && o->s_com_g1 && o->s_transcript && o->f_com_g1 && o->f_com_fr && o->f_transcript; }
// BivariatePolynomialCommitment::open (transparent.rs:129-186) on a dense coefficient matrix in device memory
static int32_t tpc_open_dev(Engine* e, const ripp_tpc_ck* s, const Fr* dcoef, size_t rows, size_t cols, size_t stride, const ripp_g1j* y_coms, const Fr& x, const Fr& y,
                            ripp_tpc_opening* o, ripp_fr* eval, ripp_stats* st) {
    const TwoTier k = tpc_key(s); const size_t nx = k.nx, ny = k.ny; int32_t rc;
    std::vector<Fr> yp;
    SsmVecs v; G1J yc; Fr ev; double t_start;
    rc = two_tier_open_prefix(e, k, v, dcoef, rows, cols, stride, x, &yc, &t_start, [&]() -> int32_t {                   // :141-159; behind the powers of x, those of y (:170-174)
        int32_t r1 = tpc_reserve_first(e, ny); if (r1) return r1;
        yp = fr_powers(y, ny);
        HIPCHK(hipMemcpyAsync(e->tpc_b.p, yp.data(), ny * sizeof(Fr), hipMemcpyHostToDevice, e->stream));
        return RIPP_OK; });
    if (rc) return rc;
    if ((rc = fr_dot_dev(e, e->pc_yev.as<Fr>(), e->tpc_b.as<Fr>(), ny, &ev))) return rc;                               // p(x, y) = <y_eval_coeffs, powers of y>
    // second tier over (y_polynomial_comms, powers of x) under second_tier_ck (:161-168)
    if ((rc = two_tier_load_second(e, k, v, y_coms))) return rc;
    G1A ha; Fr hs; G2A hka; size_t r2 = 0;
    if ((rc = tipa_ssm_rounds(e, v, nx, o->s_com_gt, o->s_com_g1, o->s_transcript, ha, hs, hka, &r2))) return rc;
    // first tier over (y_eval_coeffs, powers of y) under first_tier_ck (:176-183): the coefficients never left the device
    HIPCHK(hipMemcpyAsync(e->tpc_m.p, e->pc_yev.p, ny * sizeof(Fr), hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->tpc_k.p, k.bases, ny * sizeof(G1A), hipMemcpyDeviceToDevice, e->stream));
    Fr fa, fb;
    if ((rc = tpc_scalar_rounds(e, ny, k.ext, o->f_com_g1, o->f_com_fr, o->f_transcript, fa, fb))) return rc;
    const G1J ja = to_jac(ha);
    std::memcpy(&o->s_base_a, &ja, sizeof ja); std::memcpy(&o->s_base_b, &hs, sizeof hs); std::memcpy(&o->y_eval_comm, &yc, sizeof yc);
    std::memcpy(&o->f_base_a, &fa, sizeof fa); std::memcpy(&o->f_base_b, &fb, sizeof fb);
    if (eval) std::memcpy(eval, &ev, sizeof ev);
    return finish_stats(e, t_start, st);
}
// BivariatePolynomialCommitment::verify (transparent.rs:188-212)
static int32_t tpc_verify_core(Engine* e, const ripp_tpc_ck* s, const ripp_gt* com, const Fr& x, const Fr& y, const Fr& eval, const ripp_tpc_opening* o, int32_t* accept) {
    const TwoTier k = tpc_key(s); int32_t rc; bool ok2 = false, ok1 = false;
    const G1J yc = load_jac<Fp>(&o->y_eval_comm);
    if ((rc = tpc_mexp_verify_core(e, k.ck, log2_sz(k.nx), load_gt(com), yc, x, o->s_com_gt, o->s_com_g1, load_jac<Fp>(&o->s_base_a), load_fr(&o->s_base_b), &ok2))) return rc;
    if ((rc = tpc_scalar_verify_core(e, k.bases, log2_sz(k.ny), yc, eval, y, o->f_com_g1, o->f_com_fr, load_fr(&o->f_base_a), load_fr(&o->f_base_b), &ok1))) return rc;
    *accept = (ok2 && ok1) ? 1 : 0; return RIPP_OK;
}
}  // extern "C++"

// BivariatePolynomialCommitment::commit (transparent.rs:101-127): the coefficient-matrix convention of ripp_pc_commit
API int32_t ripp_tpc_commit(const ripp_tpc_ck* s, const ripp_fr* coeffs, size_t rows, size_t cols, size_t stride, ripp_gt* com, ripp_g1j* y_coms) {
    if (!s || !com || !y_coms || (rows && cols && !coeffs) || stride < cols) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    int32_t rc; Fr* dc;
    if ((rc = two_tier_fits("ripp_tpc_commit", "the key's degrees", tpc_key(s), rows, cols)) || (rc = pc_upload_matrix(e, coeffs, rows, cols, stride, &dc))) return rc;
    return two_tier_commit(e, tpc_key(s), dc, rows, cols, cols, com, y_coms);
}
// BivariatePolynomialCommitment::open (transparent.rs:129-186)
API int32_t ripp_tpc_open(const ripp_tpc_ck* s, const ripp_fr* coeffs, size_t rows, size_t cols, size_t stride, const ripp_g1j* y_coms, const ripp_fr* x, const ripp_fr* y,
                          ripp_tpc_opening* opening, ripp_fr* eval, ripp_stats* st) {
    if (!s || !y_coms || !x || !y || !tpc_opening_ok(opening) || (rows && cols && !coeffs) || stride < cols) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    int32_t rc; Fr* dc;
    if ((rc = two_tier_fits("ripp_tpc_open", "the key's degrees", tpc_key(s), rows, cols)) || (rc = pc_upload_matrix(e, coeffs, rows, cols, stride, &dc))) return rc;
    return tpc_open_dev(e, s, dc, rows, cols, cols, y_coms, load_fr(x), load_fr(y), opening, eval, st);
}
// BivariatePolynomialCommitment::verify (transparent.rs:188-212)
API int32_t ripp_tpc_verify(const ripp_tpc_ck* s, const ripp_gt* com, const ripp_fr* x, const ripp_fr* y, const ripp_fr* eval, const ripp_tpc_opening* opening, int32_t* accept) {
    if (!s || !com || !x || !y || !eval || !tpc_opening_ok(opening) || !accept) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    return tpc_verify_core(e, s, com, load_fr(x), load_fr(y), load_fr(eval), opening, accept);
}
// UnivariatePolynomialCommitment (transparent.rs:235-330): the flat coefficient array with stride y_degree + 1, the point (z^(y_degree + 1), z)
API int32_t ripp_tpc_commit_univariate(const ripp_tpc_ck* s, const ripp_fr* coeffs, size_t len, ripp_gt* com, ripp_g1j* y_coms) {
    if (!s || !com || !y_coms || (len && !coeffs)) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    len = pc_stripped_len(coeffs, len);
    int32_t rc; Fr* dc; size_t rows;
    if ((rc = two_tier_flat_fits("ripp_tpc_commit_univariate", "the key's", tpc_key(s), len)) || (rc = pc_upload_flat(e, coeffs, len, s->ny, &rows, &dc))) return rc;
    return two_tier_commit(e, tpc_key(s), dc, rows, rows ? s->ny : 0, s->ny, com, y_coms);
}
API int32_t ripp_tpc_open_univariate(const ripp_tpc_ck* s, const ripp_fr* coeffs, size_t len, const ripp_g1j* y_coms, const ripp_fr* point, ripp_tpc_opening* opening, ripp_fr* eval, ripp_stats* st) {
    if (!s || !y_coms || !point || !tpc_opening_ok(opening) || (len && !coeffs)) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    len = pc_stripped_len(coeffs, len);
    int32_t rc; Fr* dc; size_t rows;
    if ((rc = two_tier_flat_fits("ripp_tpc_open_univariate", "the key's", tpc_key(s), len)) || (rc = pc_upload_flat(e, coeffs, len, s->ny, &rows, &dc))) return rc;
    const Fr z = load_fr(point);
    return tpc_open_dev(e, s, dc, rows, rows ? s->ny : 0, s->ny, y_coms, fr_pow_u(z, s->ny), z, opening, eval, st);               // :283-290
}
API int32_t ripp_tpc_verify_univariate(const ripp_tpc_ck* s, const ripp_gt* com, const ripp_fr* point, const ripp_fr* eval, const ripp_tpc_opening* opening, int32_t* accept) {
    if (!s || !com || !point || !eval || !tpc_opening_ok(opening) || !accept) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    const Fr z = load_fr(point);
    return tpc_verify_core(e, s, com, fr_pow_u(z, s->ny), z, load_fr(eval), opening, accept);                                    // :314-321
}

// ---- the two tier arguments on their own, from host slices ---------------------------------------------------------------------------------
// first tier: GIPAWithSSM<ScalarInnerProduct, PedersenCommitment<G1>, IdentityCommitment<Fr>>::prove_with_structured_scalar_message (ssm.rs:66-84)
API int32_t ripp_gipa_ssm_scalar_prove(const ripp_fr* m, const ripp_fr* b, const ripp_g1a* ck, size_t n, ripp_g1j* com_g1, ripp_fr* com_fr, ripp_fr* transcript,
                                       ripp_fr* base_a, ripp_fr* base_b, ripp_stats* st) {
    if (n < 2 || !is_pow2(n) || n > ((size_t)1 << 28)) return RIPP_ERR_POW2;
    if (!m || !b || !ck || !com_g1 || !com_fr || !transcript || !base_a || !base_b) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    e->stats = ripp_stats{};
    const double t_start = now_ms();
    int32_t rc; if ((rc = tpc_reserve_first(e, n))) return rc;
    HIPCHK(hipMemcpyAsync(e->tpc_m.p, m, n * sizeof(Fr), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->tpc_b.p, b, n * sizeof(Fr), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->tpc_k.p, ck, n * sizeof(G1A), hipMemcpyHostToDevice, e->stream));
    Fr fa, fb;
    if ((rc = tpc_scalar_rounds(e, n, nullptr, com_g1, com_fr, transcript, fa, fb))) return rc;
    std::memcpy(base_a, &fa, sizeof fa); std::memcpy(base_b, &fb, sizeof fb);
    return finish_stats(e, t_start, st);
}
// ... ::verify_with_structured_scalar_message (ssm.rs:86-127); com = (com_a: Pedersen commitment of the message, com_t: the inner product)
API int32_t ripp_gipa_ssm_scalar_verify(const ripp_g1a* ck, size_t n, const ripp_g1j* com_a, const ripp_fr* com_t, const ripp_fr* scalar_b,
                                        const ripp_g1j* com_g1, const ripp_fr* com_fr, const ripp_fr* base_a, const ripp_fr* base_b, int32_t* accept) {
    if (n < 2 || !is_pow2(n) || n > ((size_t)1 << 28)) return RIPP_ERR_POW2;
    if (!ck || !com_a || !com_t || !scalar_b || !com_g1 || !com_fr || !base_a || !base_b || !accept) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    G1A* dk; int32_t rc; bool ok = false;
    if ((rc = upload<G1A>(e, e->affG1, ck, n, &dk))) return rc;
    if ((rc = tpc_scalar_verify_core(e, dk, log2_sz(n), load_jac<Fp>(com_a), load_fr(com_t), load_fr(scalar_b), com_g1, com_fr, load_fr(base_a), load_fr(base_b), &ok))) return rc;
    *accept = ok ? 1 : 0; return RIPP_OK;
}
// second tier: GIPAWithSSM<MultiexponentiationInnerProduct<G1>, AFGHOCommitmentG1, IdentityCommitment<G1>>::prove_with_structured_scalar_message
API int32_t ripp_gipa_ssm_mexp_prove(const ripp_g1j* m, const ripp_fr* b, const ripp_g2a* ck, size_t n, ripp_gt* com_gt, ripp_g1j* com_g1, ripp_fr* transcript,
                                     ripp_g1j* base_a, ripp_fr* base_b, ripp_stats* st) {
    if (n < 2 || !is_pow2(n) || n > ((size_t)1 << 24)) return RIPP_ERR_POW2;
    if (!m || !b || !ck || !com_gt || !com_g1 || !transcript || !base_a || !base_b) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    e->stats = ripp_stats{};
    const double t_start = now_ms();
    SsmVecs v; int32_t rc; if ((rc = v.reserve(n))) return rc;
    if ((rc = ssm_load_message(e, v, m, n))) return rc;
    HIPCHK(hipMemcpyAsync(v.KA.p, ck, n * sizeof(G2A), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(v.S.p, b, n * sizeof(Fr), hipMemcpyHostToDevice, e->stream)); if ((rc = e->sync())) return rc;
    G1A ha; Fr hs; G2A hka; size_t rounds = 0;
    if ((rc = tipa_ssm_rounds(e, v, n, com_gt, com_g1, transcript, ha, hs, hka, &rounds))) return rc;
    const G1J ja = to_jac(ha);
    std::memcpy(base_a, &ja, sizeof ja); std::memcpy(base_b, &hs, sizeof hs);
    return finish_stats(e, t_start, st);
}
// ... ::verify_with_structured_scalar_message; com = (com_a in GT: AFGHO commitment of the message, com_t in G1: the inner product)
API int32_t ripp_gipa_ssm_mexp_verify(const ripp_g2a* ck, size_t n, const ripp_gt* com_a, const ripp_g1j* com_t, const ripp_fr* scalar_b,
                                      const ripp_gt* com_gt, const ripp_g1j* com_g1, const ripp_g1j* base_a, const ripp_fr* base_b, int32_t* accept) {
    if (n < 2 || !is_pow2(n) || n > ((size_t)1 << 24)) return RIPP_ERR_POW2;
    if (!ck || !com_a || !com_t || !scalar_b || !com_gt || !com_g1 || !base_a || !base_b || !accept) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    G2A* dk; int32_t rc; bool ok = false;
    if ((rc = upload<G2A>(e, e->affG2, ck, n, &dk))) return rc;
    if ((rc = tpc_mexp_verify_core(e, dk, log2_sz(n), load_gt(com_a), load_jac<Fp>(com_t), load_fr(scalar_b), com_gt, com_g1, load_jac<Fp>(base_a), load_fr(base_b), &ok))) return rc;
    *accept = ok ? 1 : 0; return RIPP_OK;
}
