// Included by engine.hip inside its `extern "C"` block, after tpc_api.inc.
// GIPA<MultiexponentiationInnerProduct<G1>, AFGHOCommitmentG1, PedersenCommitment<G1>, IdentityCommitment<G1>, Blake2b>: the MIPP argument with an arbitrary,
// COMMITTED scalar vector (ip_proofs/src/gipa.rs:499-530, benches/benches/gipa.rs case 2).  m_a in G1, m_b in Fr, ck_a in G2 (AFGHO), ck_b in G1 (Pedersen).
// Per round (gipa.rs:207-291), h = len / 2:
//     com_1 = (AFGHO(ck_a[:h], m_a[h:]), <ck_b[h:], m_b[:h]>, <m_a[h:], m_b[:h]>)      com_2 = (AFGHO(ck_a[h:], m_a[:h]), <ck_b[:h], m_b[h:]>, <m_a[:h], m_b[h:]>)
//     m_a <- c m_a[h:] + m_a[:h]      m_b <- c^-1 m_b[h:] + m_b[:h]      ck_a <- c^-1 ck_a[h:] + ck_a[:h]      ck_b <- c ck_b[h:] + ck_b[:h]
// The pairing half and the m_a / m_b / ck_a folds are those of tipa_ssm_rounds.  New: the four G1 MSMs of the round.  ck_b and m_a are kept side by side in ONE
// buffer X = (ck_b | m_a) and the two folds write side by side into the next round's X, so that from vector length e->cfg.gipa_mexp_batch_min on the four MSMs are
// the four rows of one pass of the batched pipeline over X (gipa_mexp.hpp); below it, and under the legacy MSM switches, four single MSMs, two on each side stream.
extern "C++" {
struct MexpVecs {
    DevBuf X, X2, S, S2, KA, KA2, jacA, jacK, jac2, qt2, out;
    FoldPre pA, pKB, pKA;                   // second fold bases of the small rounds
    VecLease lease{&g_mexp_cache, {&X, &X2, &S, &S2, &KA, &KA2, &jacA, &jacK, &jac2, &qt2, &out, &pA.pow_h, &pA.parts, &pKB.pow_h, &pKB.parts, &pKA.pow_h, &pKA.parts}};      // (last member)
    int32_t reserve(size_t n) {
        int32_t rc;
        if ((rc = X.reserve(2 * n * sizeof(G1A))) || (rc = X2.reserve(2 * n * sizeof(G1A))) || (rc = S.reserve(n * sizeof(Fr))) || (rc = S2.reserve(n * sizeof(Fr))) ||
            (rc = KA.reserve(n * sizeof(G2A))) || (rc = KA2.reserve(n * sizeof(G2A))) || (rc = jacA.reserve(n * sizeof(G1J))) || (rc = jacK.reserve(n * sizeof(G1J))) ||
            (rc = jac2.reserve(n * sizeof(G2J))) || (rc = out.reserve(4 * sizeof(G1J)))) return rc;
        return RIPP_OK;
    }
};
// reserve v for n elements and load an instance from the host: m_a normalised into the upper half of v.X, ck_b below it, ck_a and m_b as they come
static int32_t mexp_upload(Engine* e, MexpVecs& v, const ripp_g1j* m_a, const ripp_fr* m_b, const ripp_g2a* ck_a, const ripp_g1a* ck_b, size_t n) {
    int32_t rc; if ((rc = v.reserve(n))) return rc;
    HIPCHK(hipMemcpyAsync(v.jacA.p, m_a, n * sizeof(G1J), hipMemcpyHostToDevice, e->stream));
    if ((rc = e->normalize_dev<Fp>(v.jacA.as<G1J>(), n, v.X.as<G1A>() + n))) return rc;
    HIPCHK(hipMemcpyAsync(v.X.p, ck_b, n * sizeof(G1A), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(v.KA.p, ck_a, n * sizeof(G2A), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(v.S.p, m_b, n * sizeof(Fr), hipMemcpyHostToDevice, e->stream));
    return e->sync();
}

// GIPA::_prove (gipa.rs:181-312) on v.X = (ck_b | m_a), v.S = m_b, v.KA = ck_a, n elements each, resident and affine.  Steps and transcript in ROUND order.
static int32_t gipa_mexp_rounds(Engine* e, MexpVecs& v, size_t n, ripp_gt* com_gt, ripp_g1j* com_ped, ripp_g1j* com_ip, ripp_fr* transcript,
                                G1A& ha, Fr& hs, G2A& hka, G1A& hkb) {
    int32_t rc;
    size_t len = n, round = 0;
    Fr prev_c = Fr::zero();
    std::vector<Fp12> rows(2 * N_LINES);
    while (len > 1) {
        const size_t h = len / 2;
        const G1A* KB = v.X.as<G1A>(); const G1A* A = KB + len; const G2A* KA = v.KA.as<G2A>(); const Fr* S = v.S.as<Fr>();
        G1A* KBn = v.X2.as<G1A>(); G1A* An = KBn + h;                                        // the next round's X = (ck_b | m_a), h elements each
        const G1A* as[2] = {A + h, A}; const G2A* bs[2] = {KA, KA + h};                      // com_1.0 = (m_a_1, ck_a_1), com_2.0 = (m_a_2, ck_a_2)   gipa.rs:209-231
        G1J* const out = v.out.as<G1J>();                                                    // com_1.1, com_1.2, com_2.1, com_2.2
        const bool batch = !e->msm_batch_legacy() && len >= e->cfg.gipa_mexp_batch_min && e->msm_quad_fits(len);
        const double tp = now_ms();
        if (batch) {            // one digit pass and one sort for the four MSMs, in front of the pairing products on the engine's stream
            if ((rc = e->msm_batch_dev<Fp>(KB, nullptr, S, 4, 2 * len, 0, out, 0, (uint32_t)len))) return rc;
        } else {                // two MSMs after one another on each side stream, beside the pairing products; each scratch is reused in stream order
            struct { hipStream_t st; int ms; const G1A* b; const Fr* s; } q[4] = {{e->stream2, 0, KB + h, S}, {e->stream3, 1, A + h, S}, {e->stream2, 0, KB, S + h}, {e->stream3, 1, A, S + h}};
            for (int k = 0; k < 4; ++k) {
                if ((rc = e->msm_launch<Fp>(e->msm_scratch[q[k].ms], q[k].st, q[k].b, q[k].s, h))) return rc;
                HIPCHK(hipMemcpyAsync(out + k, e->msm_scratch[q[k].ms].out.p, sizeof(G1J), hipMemcpyDeviceToDevice, q[k].st));
            }
        }
        if ((rc = e->step_products(as, bs, 2, h, rows.data()))) return rc;
        if (!batch) { HIPCHK(hipStreamSynchronize(e->stream2)); HIPCHK(hipStreamSynchronize(e->stream3)); }
        G1J cm[4];
        HIPCHK(hipMemcpyAsync(cm, out, sizeof cm, hipMemcpyDeviceToHost, e->stream)); if ((rc = e->sync())) return rc;
        // small rounds: the second bases of the three group folds during the host phase
        if ((rc = fold_precompute<Fp>(e, e->stream2, A + h, h, v.pA)) || (rc = fold_precompute<Fp>(e, e->stream3, KB + h, h, v.pKB)) || (rc = fold_precompute<Fp2>(e, e->stream, KA + h, h, v.pKA))) return rc;
        e->stats.miller_products_ms += now_ms() - tp;
        const double th = now_ms();
        Fp12 gt[2];
        { auto fut = host_pool().submit([&rows]() { return final_exponentiation(miller_combine(rows.data() + N_LINES)); });
          gt[0] = final_exponentiation(miller_combine(rows.data())); gt[1] = fut.get(); }
        const G1J ped[2] = {cm[0], cm[2]}, ip[2] = {cm[1], cm[3]};
        const G1A peda[2] = {to_affine(ped[0]), to_affine(ped[1])}, ipa[2] = {to_affine(ip[0]), to_affine(ip[1])};
        Fr c_inv; const Fr c = fs::gipa_challenge(round ? &prev_c : nullptr, fs::Com{gt[0], peda[0], ipa[0]}, fs::Com{gt[1], peda[1], ipa[1]}, c_inv);
        e->stats.host_ms += now_ms() - th;
        std::memcpy(&com_gt[2 * round], gt, sizeof gt); std::memcpy(&com_ped[2 * round], ped, sizeof ped); std::memcpy(&com_ip[2 * round], ip, sizeof ip);
        std::memcpy(&transcript[round], &c, sizeof c);
        prev_c = c;
        const double tf = now_ms();
        rc = fork_join_folds(e, [&]() -> int32_t {
            int32_t r2;
            if ((r2 = fold_dev<Fp>(e, e->stream2, A + h, A, h, c, v.jacA, v.qt2, An, &v.pA))) return r2;                              // m_a  <- m_a_1 * c + m_a_2
            if ((r2 = fold_dev<Fp>(e, e->stream3, KB + h, KB, h, c, v.jacK, v.qt2, KBn, &v.pKB))) return r2;                          // ck_b <- ck_b_1 * c + ck_b_2   (ck_b_1 = ck_b[h:], gipa.rs:216)
            hipLaunchKernelGGL(k_fold_fr, dim3(nblk(h, 256)), dim3(256), 0, e->stream4, S + h, S, (uint32_t)h, c_inv, v.S2.as<Fr>());   // m_b  <- m_b_2 * c_inv + m_b_1
            HIPCHK(hipGetLastError());
            return fold_dev<Fp2>(e, e->stream, KA + h, KA, h, c_inv, v.jac2, e->qtab, v.KA2.as<G2A>(), &v.pKA);                        // ck_a <- ck_a_2 * c_inv + ck_a_1
        });
        if (rc) return rc;
        e->stats.fold_ms += now_ms() - tf;
        std::swap(v.X, v.X2); std::swap(v.S, v.S2); std::swap(v.KA, v.KA2);
        len = h; ++round;
    }
    HIPCHK(hipMemcpy(&hkb, v.X.p, sizeof hkb, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(&ha, v.X.as<G1A>() + 1, sizeof ha, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&hs, v.S.p, sizeof hs, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(&hka, v.KA.p, sizeof hka, hipMemcpyDeviceToHost));
    return RIPP_OK;
}

// _compute_recursive_challenges (gipa.rs:322-363) for this instantiation: folds the steps into (ca, cb, ct) = (com_a, com_b, com_t); tr in ROUND order
static bool gipa_mexp_replay(Fp12& ca, G1J& cb, G1J& ct, const ripp_gt* com_gt, const ripp_g1j* com_ped, const ripp_g1j* com_ip, size_t rounds, std::vector<Fr>& tr) {
    return gipa_replay<Fp12, G1A, G1A>(ca, cb, ct, rounds, tr, [&](size_t k, auto& s1, auto& s2) {
        s1 = {load_gt(&com_gt[2 * k]), load_g1a(&com_ped[2 * k]), load_g1a(&com_ip[2 * k])}; s2 = {load_gt(&com_gt[2 * k + 1]), load_g1a(&com_ped[2 * k + 1]), load_g1a(&com_ip[2 * k + 1])}; });
}
}  // extern "C++"

API int32_t ripp_gipa_mexp_prove(const ripp_g1j* m_a, const ripp_fr* m_b, const ripp_g2a* ck_a, const ripp_g1a* ck_b, size_t n,
                                 ripp_gt* com_gt, ripp_g1j* com_ped, ripp_g1j* com_ip, ripp_fr* transcript,
                                 ripp_g1j* base_a, ripp_fr* base_b, ripp_g2j* ck_base_a, ripp_g1j* ck_base_b, ripp_stats* st) {
    if (n < 2 || !is_pow2(n) || n > ((size_t)1 << 24)) return RIPP_ERR_POW2;
    if (!m_a || !m_b || !ck_a || !ck_b || !com_gt || !com_ped || !com_ip || !transcript || !base_a || !base_b || !ck_base_a || !ck_base_b) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    e->stats = ripp_stats{};
    const double t_start = now_ms();
    MexpVecs v; int32_t rc; if ((rc = mexp_upload(e, v, m_a, m_b, ck_a, ck_b, n))) return rc;
    G1A ha, hkb; Fr hs; G2A hka;
    if ((rc = gipa_mexp_rounds(e, v, n, com_gt, com_ped, com_ip, transcript, ha, hs, hka, hkb))) return rc;
    const G1J ja = to_jac(ha), jkb = to_jac(hkb); const G2J jka = to_jac(hka);
    std::memcpy(base_a, &ja, sizeof ja); std::memcpy(base_b, &hs, sizeof hs); std::memcpy(ck_base_a, &jka, sizeof jka); std::memcpy(ck_base_b, &jkb, sizeof jkb);
    return finish_stats(e, t_start, st);
}

API int32_t ripp_gipa_mexp_verify(const ripp_g2a* ck_a, const ripp_g1a* ck_b, size_t n,
                                  const ripp_gt* com_a, const ripp_g1j* com_b, const ripp_g1j* com_t,
                                  const ripp_gt* com_gt, const ripp_g1j* com_ped, const ripp_g1j* com_ip,
                                  const ripp_g1j* base_a, const ripp_fr* base_b, int32_t* accept) {
    if (n < 2 || !is_pow2(n) || n > ((size_t)1 << 24)) return RIPP_ERR_POW2;
    if (!ck_a || !ck_b || !com_a || !com_b || !com_t || !com_gt || !com_ped || !com_ip || !base_a || !base_b || !accept) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    Fp12 ca = load_gt(com_a); G1J cb = load_jac<Fp>(com_b), ct = load_jac<Fp>(com_t);
    std::vector<Fr> tr;
    if (!gipa_mexp_replay(ca, cb, ct, com_gt, com_ped, com_ip, log2_sz(n), tr)) { *accept = 0; return RIPP_OK; }
    // _compute_final_commitment_keys (gipa.rs:365-399) as one device MSM per key: powers of c^-1 for ck_a, of c for ck_b
    G2A* dka; G1A* dkb; G2J ka; G1J kb; int32_t rc;
    if ((rc = upload<G2A>(e, e->affG2, ck_a, n, &dka)) || (rc = tpc_final_key<Fp2>(e, dka, final_key_exponents(tr, true), &ka))) return rc;
    if ((rc = upload<G1A>(e, e->affG1, ck_b, n, &dkb)) || (rc = tpc_final_key<Fp>(e, dkb, final_key_exponents(tr, false), &kb))) return rc;
    // _verify_base_commitment (gipa.rs:401-415)
    const G1A a = to_affine(load_jac<Fp>(base_a)); const Fr b = load_fr(base_b);
    Fp12 e1; if ((rc = pairing_host_pts(e, {a}, {to_affine(ka)}, &e1))) return rc;
    *accept = (e1 == ca && eq(smul_host(to_affine(kb), b), cb) && eq(smul_host(a, b), ct)) ? 1 : 0;
    return RIPP_OK;
}
