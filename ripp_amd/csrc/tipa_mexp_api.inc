// Included by engine.hip inside its `extern "C"` block, after gipa_mexp_api.inc.
// TIPA<MultiexponentiationInnerProduct<G1>, AFGHOCommitmentG1, PedersenCommitment<G1>, IdentityCommitment<G1>, Blake2b> (ip_proofs/src/tipa/mod.rs:473-497,
// benches/benches/tipa.rs case 2): the MIPP argument with an arbitrary, COMMITTED scalar vector and a logarithmic verifier.  The prover
// (TIPA::prove_with_srs_shift, mod.rs:176-231) is the round loop of gipa_mexp_api.inc followed by the KZG openings of both final keys (tipp_kzg, tipa_api.inc);
// the verifier (verify_with_srs_shift, mod.rs:233-301) replays the steps, checks both openings and the base commitments and never sees the keys.

API int32_t ripp_tipa_mexp_prove(const ripp_srs* srs, const ripp_g1j* m_a, const ripp_fr* m_b, const ripp_g2a* ck_a, const ripp_g1a* ck_b, size_t n,
                                 const ripp_fr* r_shift, ripp_gt* com_gt, ripp_g1j* com_ped, ripp_g1j* com_ip, ripp_fr* transcript,
                                 ripp_g1j* base_a, ripp_fr* base_b, ripp_g2j* final_ck_a, ripp_g1j* final_ck_b,
                                 ripp_g2j* opening_a, ripp_g1j* opening_b, ripp_fr* kzg_challenge, ripp_stats* st) {
    if (n < 2 || !is_pow2(n) || n > ((size_t)1 << 24)) return RIPP_ERR_POW2;
    if (!srs || !m_a || !m_b || !ck_a || !ck_b || !r_shift || !com_gt || !com_ped || !com_ip || !transcript || !base_a || !base_b || !final_ck_a || !final_ck_b ||
        !opening_a || !opening_b || !kzg_challenge) return RIPP_ERR_ARG;
    if (srs->num != 2 * n - 1) { LOCK; set_err("SRS holds " + std::to_string(srs->num) + " powers, need 2n-1 = " + std::to_string(2 * n - 1)); return RIPP_ERR_ARG; }
    LOCK; ENGINE;
    e->stats = ripp_stats{};
    const double t_start = now_ms();
    MexpVecs v; int32_t rc; if ((rc = mexp_upload(e, v, m_a, m_b, ck_a, ck_b, n))) return rc;
    G1A ha, hkb; Fr hs; G2A hka;
    if ((rc = gipa_mexp_rounds(e, v, n, com_gt, com_ped, com_ip, transcript, ha, hs, hka, hkb))) return rc;                 // mod.rs:184-188
    G2J oa; G1J ob; Fr c;
    if ((rc = tipp_kzg(e, srs, transcript, log2_sz(n), load_fr(r_shift), hka, hkb, &oa, &ob, &c))) return rc;              // mod.rs:190-223
    const G1J ja = to_jac(ha), jkb = to_jac(hkb); const G2J jka = to_jac(hka);
    std::memcpy(base_a, &ja, sizeof ja); std::memcpy(base_b, &hs, sizeof hs); std::memcpy(final_ck_a, &jka, sizeof jka); std::memcpy(final_ck_b, &jkb, sizeof jkb);
    std::memcpy(opening_a, &oa, sizeof oa); std::memcpy(opening_b, &ob, sizeof ob); std::memcpy(kzg_challenge, &c, sizeof c);
    return finish_stats(e, t_start, st);
}

API int32_t ripp_tipa_mexp_verify(const ripp_verifier_srs* v_srs, const ripp_gt* com_a, const ripp_g1j* com_b, const ripp_g1j* com_t,
                                  const ripp_gt* com_gt, const ripp_g1j* com_ped, const ripp_g1j* com_ip, size_t rounds,
                                  const ripp_g1j* base_a, const ripp_fr* base_b, const ripp_g2j* final_ck_a, const ripp_g1j* final_ck_b,
                                  const ripp_g2j* opening_a, const ripp_g1j* opening_b, const ripp_fr* r_shift, int32_t* accept) {
    if (!v_srs || !com_a || !com_b || !com_t || !com_gt || !com_ped || !com_ip || !base_a || !base_b || !final_ck_a || !final_ck_b || !opening_a || !opening_b ||
        !r_shift || !accept || rounds == 0 || rounds > 24) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    Fp12 ca = load_gt(com_a); G1J cb = load_jac<Fp>(com_b), ct = load_jac<Fp>(com_t);
    std::vector<Fr> trf;
    if (!gipa_mexp_replay(ca, cb, ct, com_gt, com_ped, com_ip, rounds, trf)) { *accept = 0; return RIPP_OK; }                // mod.rs:249-251
    G2A kaa; G1A kba; bool ok = false; int32_t rc;
    if ((rc = tipa_verify_tail(e, v_srs, trf, final_ck_a, final_ck_b, opening_a, opening_b, r_shift, kaa, kba, &ok))) return rc;   // mod.rs:252-289
    const G1A a = load_g1a(base_a); const Fr b = load_fr(base_b);
    Fp12 e1; if ((rc = pairing_host_pts(e, {a}, {kaa}, &e1))) return rc;                                                     // mod.rs:291-298
    *accept = (ok && e1 == ca && eq(smul_host(kba, b), cb) && eq(smul_host(a, b), ct)) ? 1 : 0;
    return RIPP_OK;
}
