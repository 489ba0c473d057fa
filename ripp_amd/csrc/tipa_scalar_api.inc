// Included by engine.hip inside its `extern "C"` block, after tipa_mexp_api.inc.
// TIPA<ScalarInnerProduct, PedersenCommitment<G2>, PedersenCommitment<G1>, IdentityCommitment<Fr>, Blake2b> (ip_proofs/src/tipa/mod.rs:499-526): the inner
// product of two COMMITTED scalar vectors.  m_a, m_b in Fr, ck_a in G2, ck_b in G1.  Per round (gipa.rs:207-291), h = len / 2:
//     com_1 = (<ck_a[:h], m_a[h:]> in G2, <ck_b[h:], m_b[:h]> in G1, <m_a[h:], m_b[:h]> in Fr)      com_2 = (<ck_a[h:], m_a[:h]>, <ck_b[:h], m_b[h:]>, <m_a[:h], m_b[h:]>)
//     m_a <- c m_a[h:] + m_a[:h]      m_b <- c^-1 m_b[h:] + m_b[:h]      ck_a <- c^-1 ck_a[h:] + ck_a[:h]      ck_b <- c ck_b[h:] + ck_b[:h]
// The inner products and the scalar folds are the kernels of the first tier of the transparent commitment (tpc.hpp), the key folds those of the TIPP prover.
// From key length e->cfg.tipa_scalar_cross_min on the two G2 commitments of a round are ONE crossed pass of the batched MSM pipeline in its G2 form
// (tipa_scalar.hpp) and the two G1 commitments one crossed pass of its G1 form (tpc.hpp).  Both passes use the engine's one batch scratch: they are enqueued
// on the engine's stream one after the other, the G2 pass first.  Below the bound, under the legacy MSM switches and when a pass would not fit one chunk: two
// single MSMs per group on the two side streams, each scratch reused in stream order.
extern "C++" {
struct ScalVecs {
    DevBuf MA, MA2, MB, MB2, KA, KA2, KB, KB2, jac1, jac2, qt2, part, out2, out1;
    FoldPre pKA, pKB;                       // second fold bases of the small rounds
    VecLease lease{&g_scal_cache, {&MA, &MA2, &MB, &MB2, &KA, &KA2, &KB, &KB2, &jac1, &jac2, &qt2, &part, &out2, &out1, &pKA.pow_h, &pKA.parts, &pKB.pow_h, &pKB.parts}};      // (last member)
    int32_t reserve(size_t n) {
        int32_t rc;
        for (DevBuf* b : {&MA, &MA2, &MB, &MB2}) if ((rc = b->reserve(n * sizeof(Fr)))) return rc;
        if ((rc = KA.reserve(n * sizeof(G2A))) || (rc = KA2.reserve(n * sizeof(G2A))) || (rc = KB.reserve(n * sizeof(G1A))) || (rc = KB2.reserve(n * sizeof(G1A))) ||
            (rc = jac1.reserve(n * sizeof(G1J))) || (rc = jac2.reserve(n * sizeof(G2J))) || (rc = part.reserve(2 * 1024 * sizeof(Fr))) ||
            (rc = out2.reserve(2 * sizeof(G2J))) || (rc = out1.reserve(2 * sizeof(G1J)))) return rc;
        return RIPP_OK;
    }
};

// GIPA::_prove (gipa.rs:181-312) on v.MA, v.MB, v.KA, v.KB, n elements each, resident (keys affine).  com_g2[r][2] = (com_1.0, com_2.0), com_g1[r][2] = (com_1.1, com_2.1),
// com_fr[r][2] = (com_1.2[0], com_2.2[0]), transcript[r]: ROUND order.
static int32_t tipa_scalar_rounds(Engine* e, ScalVecs& v, size_t n, ripp_g2j* com_g2, ripp_g1j* com_g1, ripp_fr* com_fr, ripp_fr* transcript,
                                  Fr& ha, Fr& hb, G2A& hka, G1A& hkb) {
    int32_t rc;
    size_t len = n, round = 0;
    Fr prev_c = Fr::zero();
    FrDot2 dot;
    while (len > 1) {
        const size_t h = len / 2;
        const Fr* MA = v.MA.as<Fr>(); const Fr* MB = v.MB.as<Fr>(); const G2A* KA = v.KA.as<G2A>(); const G1A* KB = v.KB.as<G1A>();
        G2J* const out2 = v.out2.as<G2J>(); G1J* const out1 = v.out1.as<G1J>();              // (com_1.0, com_2.0), (com_1.1, com_2.1)
        const bool cross = !e->msm_batch_legacy() && len >= e->cfg.tipa_scalar_cross_min && e->msm_rows_fit<Fp2>(len, 2) && e->msm_rows_fit<Fp>(len, 2);
        const double tp = now_ms();
        if (cross) {
            // rows 0, 1 over ck_a with m_a: <ck_a[:h], m_a[h:]> = com_1.0, <ck_a[h:], m_a[:h]> = com_2.0   (gipa.rs:209-231)
            if ((rc = e->msm_batch_dev<Fp2>(KA, nullptr, MA, 2, len, 0, out2, (uint32_t)h))) return rc;
            // rows 0, 1 over ck_b with m_b: <ck_b[:h], m_b[h:]> = com_2.1, <ck_b[h:], m_b[:h]> = com_1.1 -- the other way round (ck_b_1 = ck_b[h:], gipa.rs:216)
            if ((rc = e->msm_batch_dev<Fp>(KB, nullptr, MB, 2, len, 0, out1, (uint32_t)h))) return rc;
        } else {
            if ((rc = e->msm_launch<Fp2>(e->msm_scratch[0], e->stream2, KA, MA + h, h))) return rc;
            HIPCHK(hipMemcpyAsync(out2, e->msm_scratch[0].out.p, sizeof(G2J), hipMemcpyDeviceToDevice, e->stream2));
            if ((rc = e->msm_launch<Fp2>(e->msm_scratch[1], e->stream3, KA + h, MA, h))) return rc;
            HIPCHK(hipMemcpyAsync(out2 + 1, e->msm_scratch[1].out.p, sizeof(G2J), hipMemcpyDeviceToDevice, e->stream3));
            if ((rc = e->msm_launch<Fp>(e->msm_scratch[0], e->stream2, KB, MB + h, h))) return rc;
            HIPCHK(hipMemcpyAsync(out1, e->msm_scratch[0].out.p, sizeof(G1J), hipMemcpyDeviceToDevice, e->stream2));
            if ((rc = e->msm_launch<Fp>(e->msm_scratch[1], e->stream3, KB + h, MB, h))) return rc;
            HIPCHK(hipMemcpyAsync(out1 + 1, e->msm_scratch[1].out.p, sizeof(G1J), hipMemcpyDeviceToDevice, e->stream3));
        }
        if ((rc = dot.launch(e, MA, MB, h, v.part))) return rc;                                    // <m_a[h:], m_b[:h]>, <m_a[:h], m_b[h:]>
        if (!cross) { HIPCHK(hipStreamSynchronize(e->stream2)); HIPCHK(hipStreamSynchronize(e->stream3)); }
        G2J c2[2]; G1J c1[2];
        HIPCHK(hipMemcpyAsync(c2, out2, sizeof c2, hipMemcpyDeviceToHost, e->stream)); HIPCHK(hipMemcpyAsync(c1, out1, sizeof c1, hipMemcpyDeviceToHost, e->stream));
        if ((rc = e->sync())) return rc;
        std::swap(c1[0], c1[1]);                                                                  // both forms leave (com_2.1, com_1.1) in out1
        // small rounds: the second bases of the two key folds during the host phase
        if ((rc = fold_precompute<Fp2>(e, e->stream, KA + h, h, v.pKA)) || (rc = fold_precompute<Fp>(e, e->stream2, KB + h, h, v.pKB))) return rc;
        e->stats.miller_products_ms += now_ms() - tp;                                             // (no Miller loop here: the round's commitments and inner products)
        const double th = now_ms();
        Fr ip[2]; dot.sum(ip);
        Fr c_inv; const Fr c = fs::gipa_challenge(round ? &prev_c : nullptr, fs::Com{to_affine(c2[0]), to_affine(c1[0]), ip[0]}, fs::Com{to_affine(c2[1]), to_affine(c1[1]), ip[1]}, c_inv);
        e->stats.host_ms += now_ms() - th;
        std::memcpy(&com_g2[2 * round], c2, sizeof c2); std::memcpy(&com_g1[2 * round], c1, sizeof c1); std::memcpy(&com_fr[2 * round], ip, sizeof ip);
        std::memcpy(&transcript[round], &c, sizeof c);
        prev_c = c;
        const double tf = now_ms();
        rc = fork_join_folds(e, [&]() -> int32_t {
            int32_t r2;
            if ((r2 = fold_dev<Fp>(e, e->stream2, KB + h, KB, h, c, v.jac1, v.qt2, v.KB2.as<G1A>(), &v.pKB))) return r2;                 // ck_b <- ck_b_1 * c + ck_b_2   (ck_b_1 = ck_b[h:])
            hipLaunchKernelGGL(k_fold_fr2, dim3(nblk(h, 256), 2), dim3(256), 0, e->stream3, MA, MB, (uint32_t)h, c, c_inv, v.MA2.as<Fr>(), v.MB2.as<Fr>());   // m_a <- m_a_1 * c + m_a_2, m_b <- m_b_2 * c_inv + m_b_1
            HIPCHK(hipGetLastError());
            return fold_dev<Fp2>(e, e->stream, KA + h, KA, h, c_inv, v.jac2, e->qtab, v.KA2.as<G2A>(), &v.pKA);                           // ck_a <- ck_a_2 * c_inv + ck_a_1
        });
        if (rc) return rc;
        e->stats.fold_ms += now_ms() - tf;
        std::swap(v.MA, v.MA2); std::swap(v.MB, v.MB2); std::swap(v.KA, v.KA2); std::swap(v.KB, v.KB2);
        len = h; ++round;
    }
    HIPCHK(hipMemcpy(&ha, v.MA.p, sizeof ha, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(&hb, v.MB.p, sizeof hb, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&hka, v.KA.p, sizeof hka, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(&hkb, v.KB.p, sizeof hkb, hipMemcpyDeviceToHost));
    return RIPP_OK;
}

// _compute_recursive_challenges (gipa.rs:322-363) for this instantiation: folds the steps into (ca, cb, ct) = (com_a, com_b, com_t); tr in ROUND order
static void tipa_scalar_replay(G2J& ca, G1J& cb, Fr& ct, const ripp_g2j* com_g2, const ripp_g1j* com_g1, const ripp_fr* com_fr, size_t rounds, std::vector<Fr>& tr) {
    gipa_replay<G2A, G1A, Fr>(ca, cb, ct, rounds, tr, [&](size_t k, auto& s1, auto& s2) {                                     // (no GT member: nothing to reject)
        s1 = {load_g2a(&com_g2[2 * k]), load_g1a(&com_g1[2 * k]), load_fr(&com_fr[2 * k])}; s2 = {load_g2a(&com_g2[2 * k + 1]), load_g1a(&com_g1[2 * k + 1]), load_fr(&com_fr[2 * k + 1])}; });
}
}  // extern "C++"

API int32_t ripp_tipa_scalar_prove(const ripp_srs* srs, const ripp_fr* m_a, const ripp_fr* m_b, const ripp_g2a* ck_a, const ripp_g1a* ck_b, size_t n,
                                   const ripp_fr* r_shift, ripp_g2j* com_g2, ripp_g1j* com_g1, ripp_fr* com_fr, ripp_fr* transcript,
                                   ripp_fr* base_a, ripp_fr* base_b, ripp_g2j* final_ck_a, ripp_g1j* final_ck_b,
                                   ripp_g2j* opening_a, ripp_g1j* opening_b, ripp_fr* kzg_challenge, ripp_stats* st) {
    if (n < 2 || !is_pow2(n) || n > ((size_t)1 << 24)) return RIPP_ERR_POW2;
    if (!srs || !m_a || !m_b || !ck_a || !ck_b || !r_shift || !com_g2 || !com_g1 || !com_fr || !transcript || !base_a || !base_b || !final_ck_a || !final_ck_b ||
        !opening_a || !opening_b || !kzg_challenge) return RIPP_ERR_ARG;
    if (srs->num != 2 * n - 1) { LOCK; set_err("SRS holds " + std::to_string(srs->num) + " powers, need 2n-1 = " + std::to_string(2 * n - 1)); return RIPP_ERR_ARG; }
    LOCK; ENGINE;
    e->stats = ripp_stats{};
    const double t_start = now_ms();
    ScalVecs v; int32_t rc; if ((rc = v.reserve(n))) return rc;
    HIPCHK(hipMemcpyAsync(v.MA.p, m_a, n * sizeof(Fr), hipMemcpyHostToDevice, e->stream)); HIPCHK(hipMemcpyAsync(v.MB.p, m_b, n * sizeof(Fr), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(v.KA.p, ck_a, n * sizeof(G2A), hipMemcpyHostToDevice, e->stream)); HIPCHK(hipMemcpyAsync(v.KB.p, ck_b, n * sizeof(G1A), hipMemcpyHostToDevice, e->stream));
    if ((rc = e->sync())) return rc;
    Fr ha, hb; G2A hka; G1A hkb;
    if ((rc = tipa_scalar_rounds(e, v, n, com_g2, com_g1, com_fr, transcript, ha, hb, hka, hkb))) return rc;               // mod.rs:184-188
    G2J oa; G1J ob; Fr c;
    if ((rc = tipp_kzg(e, srs, transcript, log2_sz(n), load_fr(r_shift), hka, hkb, &oa, &ob, &c))) return rc;              // mod.rs:190-223
    const G2J jka = to_jac(hka); const G1J jkb = to_jac(hkb);
    std::memcpy(base_a, &ha, sizeof ha); std::memcpy(base_b, &hb, sizeof hb); std::memcpy(final_ck_a, &jka, sizeof jka); std::memcpy(final_ck_b, &jkb, sizeof jkb);
    std::memcpy(opening_a, &oa, sizeof oa); std::memcpy(opening_b, &ob, sizeof ob); std::memcpy(kzg_challenge, &c, sizeof c);
    return finish_stats(e, t_start, st);
}

API int32_t ripp_tipa_scalar_verify(const ripp_verifier_srs* v_srs, const ripp_g2j* com_a, const ripp_g1j* com_b, const ripp_fr* com_t,
                                    const ripp_g2j* com_g2, const ripp_g1j* com_g1, const ripp_fr* com_fr, size_t rounds,
                                    const ripp_fr* base_a, const ripp_fr* base_b, const ripp_g2j* final_ck_a, const ripp_g1j* final_ck_b,
                                    const ripp_g2j* opening_a, const ripp_g1j* opening_b, const ripp_fr* r_shift, int32_t* accept) {
    if (!v_srs || !com_a || !com_b || !com_t || !com_g2 || !com_g1 || !com_fr || !base_a || !base_b || !final_ck_a || !final_ck_b || !opening_a || !opening_b ||
        !r_shift || !accept || rounds == 0 || rounds > 24) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    G2J ca = load_jac<Fp2>(com_a); G1J cb = load_jac<Fp>(com_b); Fr ct = load_fr(com_t);
    std::vector<Fr> trf;
    tipa_scalar_replay(ca, cb, ct, com_g2, com_g1, com_fr, rounds, trf);                                                     // mod.rs:249-251
    G2A kaa; G1A kba; bool ok = false; int32_t rc;
    if ((rc = tipa_verify_tail(e, v_srs, trf, final_ck_a, final_ck_b, opening_a, opening_b, r_shift, kaa, kba, &ok))) return rc;   // mod.rs:252-289
    const Fr a = load_fr(base_a), b = load_fr(base_b);                                                                       // mod.rs:291-298
    *accept = (ok && eq(smul_host(kaa, a), ca) && eq(smul_host(kba, b), cb) && mul(a, b) == ct) ? 1 : 0;
    return RIPP_OK;
}
