// Included by engine.hip inside its `extern "C"` block (after vec_api.inc).
// ---- polynomial commitments: ip_proofs/src/applications/poly_commit/mod.rs on the device ------------------------------------------------
// KZG (mod.rs:50-119), BivariatePolynomialCommitment (:142-296) and UnivariatePolynomialCommitment (:298-388) behind a resident SRS handle.
// The group work is the batched shared-base MSM of msm_batch.hpp (the x_degree + 1 KZG commitments of `commit` in one pipeline), the
// single MSMs of msm.hpp over device-resident scalars, the AFGHO commitment (one pairing product) and the fused TIPAWithSSM prover
// (tipa_ssm_core); the field work -- partial evaluation, KZG quotient and evaluation -- runs in the Fr kernels of msm_batch.hpp, so a
// coefficient never meets host arithmetic and the quotient never visits the host.
// Every entry point takes LOCK once and calls the unlocked cores; none calls an exported function.

// UnivariatePolynomialCommitment::bivariate_degrees (mod.rs:299-306); host only, needs no device
API int32_t ripp_pc_univariate_degrees(size_t degree, size_t* x_degree, size_t* y_degree) { return sqrt_split(degree, 16, "ripp_pc_univariate_degrees", "mod.rs:302-305", x_degree, y_degree); }

extern "C++" {
// ---- the two-tier core, shared with the transparent scheme (tpc_api.inc) ------------------------------------------------------------------------
// A resident two-tier key as both schemes see it: ny first-tier G1 bases (KZG powers / Pedersen keys) with their extended GLV form for the batched MSM,
// and the nx second-tier G2 keys of the AFGHO commitment.  pc_key / tpc_key build one from a handle.
struct TwoTier { const G1A* bases; QAff<Fp>* ext; const G2A* ck; size_t nx, ny; };
// the extended form once the bases are in place
static int32_t two_tier_extend(Engine* e, const TwoTier& k) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msm_extend_q<Fp>), dim3(nblk(k.ny, 256), 2), dim3(256), 0, e->stream, k.bases, (uint32_t)k.ny, 2, k.ext);
    HIPCHK(hipGetLastError());
    return RIPP_OK;
}
// rows x cols coefficients resp. a flat array of len against the degrees of a key; noun: what the key is called in the error text
static int32_t two_tier_fits(const char* who, const char* noun, const TwoTier& k, size_t rows, size_t cols) {
    if (rows <= k.nx && cols <= k.ny) return RIPP_OK;
    set_err(std::string(who) + ": " + std::to_string(rows) + " x " + std::to_string(cols) + " coefficients exceed " + noun + " (" + std::to_string(k.nx - 1) + ", " + std::to_string(k.ny - 1) + ")");
    return RIPP_ERR_ARG;
}
static int32_t two_tier_flat_fits(const char* who, const char* noun, const TwoTier& k, size_t len) {
    if (len <= k.nx * k.ny) return RIPP_OK;
    set_err(std::string(who) + ": degree " + std::to_string(len - 1) + " exceeds " + noun + " " + std::to_string(k.nx * k.ny - 1)); return RIPP_ERR_ARG;
}
// commit (mod.rs:174-196, transparent.rs:101-127): the x_degree + 1 first-tier commitments of the rows (one batched MSM; missing rows are zero polynomials) in e->pc_out,
// then their AFGHO commitment
static int32_t two_tier_commit(Engine* e, const TwoTier& k, const Fr* dcoef, size_t rows, size_t cols, size_t stride, ripp_gt* com, ripp_g1j* y_coms) {
    int32_t rc;
    if ((rc = e->pc_out.reserve(k.nx * sizeof(G1J))) || (rc = e->pc_aff.reserve(k.nx * sizeof(G1A)))) return rc;
    HIPCHK(hipMemsetAsync(e->pc_out.p, 0, k.nx * sizeof(G1J), e->stream));            // Z = 0: the identity
    if ((rc = e->msm_batch_dev<Fp>(k.bases, cols == k.ny ? k.ext : nullptr, dcoef, rows, cols, stride, e->pc_out.as<G1J>()))) return rc;
    HIPCHK(hipMemcpyAsync(y_coms, e->pc_out.p, k.nx * sizeof(G1J), hipMemcpyDeviceToHost, e->stream));
    if ((rc = e->normalize_dev<Fp>(e->pc_out.as<G1J>(), k.nx, e->pc_aff.as<G1A>()))) return rc;
    if ((rc = e->sync())) return rc;
    return pairing_product_dev(e, e->pc_aff.as<G1A>(), k.ck, k.nx, com);
}
// the head of open (mod.rs:198-240, transparent.rs:129-159) on a dense coefficient matrix in device memory: the statistics start over (*t_start), the powers of x go
// into v.S (structured_scalar_power), y_eval_coeffs = the partial evaluation at x into e->pc_yev, *yc = y_eval_comm.  more(): what a scheme enqueues behind the powers of x.
template <class More> static int32_t two_tier_open_prefix(Engine* e, const TwoTier& k, SsmVecs& v, const Fr* dcoef, size_t rows, size_t cols, size_t stride, const Fr& x,
                                                          G1J* yc, double* t_start, More&& more) {
    int32_t rc;
    e->stats = ripp_stats{};
    *t_start = now_ms();
    const std::vector<Fr> xp = fr_powers(x, k.nx);
    if ((rc = v.reserve(k.nx))) return rc;
    HIPCHK(hipMemcpyAsync(v.S.p, xp.data(), k.nx * sizeof(Fr), hipMemcpyHostToDevice, e->stream));
    if ((rc = more()) || (rc = e->pc_yev.reserve(k.ny * sizeof(Fr)))) return rc;
    hipLaunchKernelGGL(k_pc_partial_eval, dim3(nblk(k.ny, 256)), dim3(256), 0, e->stream, dcoef, (uint32_t)rows, (uint32_t)cols, stride, v.S.as<Fr>(), (uint32_t)k.ny, e->pc_yev.as<Fr>());
    HIPCHK(hipGetLastError());
    return e->msm_dev<Fp>(k.bases, e->pc_yev.as<Fr>(), k.ny, yc);                      // synchronises: xp outlives its copy
}
// the second tier's vectors: y_polynomial_comms normalised into v.A, the key into v.KA (the powers of x are in v.S already)
static int32_t two_tier_load_second(Engine* e, const TwoTier& k, SsmVecs& v, const ripp_g1j* y_coms) {
    int32_t rc; if ((rc = ssm_load_message(e, v, y_coms, k.nx))) return rc;
    HIPCHK(hipMemcpyAsync(v.KA.p, k.ck, k.nx * sizeof(G2A), hipMemcpyDeviceToDevice, e->stream));
    return e->sync();
}
}  // extern "C++"

// KZG powers g^{alpha^i}, i <= y_degree (affine, with their extended GLV form for the batched MSM), the second-tier SRS over h^{beta^i},
// i <= 2 x_degree (the G1 side of that ripp_srs holds g only: SRS { g_alpha_powers: vec![g], .. }, mod.rs:165-170), its even powers as the
// AFGHO commitment key, and the verifier key.
struct ripp_pc_srs { DevBuf powers, ext, ck; ripp_srs ip; size_t nx = 0, ny = 0; G1J g, g_beta; G2J h, h_alpha; };

extern "C++" {
static TwoTier pc_key(const ripp_pc_srs* s) { return {static_cast<const G1A*>(s->powers.p), static_cast<QAff<Fp>*>(s->ext.p), static_cast<const G2A*>(s->ck.p), s->nx, s->ny}; }
static void pc_srs_free(ripp_pc_srs* s) { s->powers.release(); s->ext.release(); s->ck.release(); s->ip.gap.release(); s->ip.hbp.release(); delete s; }
// the derived members once powers (ny G1A) and ip.hbp (2 nx - 1 G2A) are in place
static int32_t pc_srs_finish(Engine* e, ripp_pc_srs* s) {
    int32_t rc; const size_t num = 2 * s->nx - 1;
    s->ip.num = num;
    if ((rc = s->ext.reserve(2 * s->ny * sizeof(G1A))) || (rc = s->ck.reserve(s->nx * sizeof(G2A))) || (rc = s->ip.gap.reserve(num * sizeof(G1A)))) return rc;
    if ((rc = two_tier_extend(e, pc_key(s)))) return rc;
    if ((rc = gather_even<G2A>(e, s->ip.hbp.as<G2A>(), s->nx, s->ck.as<G2A>()))) return rc;
    const std::vector<G1A> gs(num, to_affine(s->g));
    HIPCHK(hipMemcpyAsync(s->ip.gap.p, gs.data(), num * sizeof(G1A), hipMemcpyHostToDevice, e->stream));
    return e->sync();
}
// structured_generators_scalar_power (tipa/mod.rs:372-391) into device memory, normalised: out[i] = s^i * g
template <class F> static int32_t pc_powers_dev(Engine* e, const Affine<F>& g, const Fr& s, size_t num, Affine<F>* out) {
    const std::vector<Fr> pw = fr_powers(s, num);
    DevBuf& jac = std::is_same<F, Fp>::value ? e->jacG1 : e->jacG2; DevBuf& aff = std::is_same<F, Fp>::value ? e->affG1 : e->affG2;
    int32_t rc; Fr* dk;
    if ((rc = upload<Fr>(e, e->tmpR, pw.data(), num, &dk)) || (rc = jac.reserve(num * sizeof(Jac<F>))) || (rc = aff.reserve(sizeof(Affine<F>)))) return rc;
    HIPCHK(hipMemcpyAsync(aff.p, &g, sizeof g, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scale_pts<F>), dim3(nblk(num, 256)), dim3(256), 0, e->stream, aff.as<Affine<F>>(), 0u, dk, (uint32_t)num, jac.as<Jac<F>>());
    HIPCHK(hipGetLastError());
    if ((rc = e->normalize_dev<F>(jac.as<Jac<F>>(), num, out))) return rc;
    return e->sync();                                                                  // pw is the host source of an asynchronous copy
}
static bool pc_degrees_ok(size_t x_degree, size_t y_degree) {
    return is_pow2(x_degree + 1) && x_degree < ((size_t)1 << 24) && y_degree < ((size_t)1 << 30);
}
}  // extern "C++"

// KZG::setup (mod.rs:56-76) / BivariatePolynomialCommitment::setup (mod.rs:148-172) with the two trapdoors given instead of drawn; x_degree = 0 is a KZG-only handle
API int32_t ripp_pc_srs_setup(const ripp_fr* alpha, const ripp_fr* beta, size_t x_degree, size_t y_degree, ripp_pc_srs** out) {
    if (!alpha || !beta || !out) return RIPP_ERR_ARG;
    if (!pc_degrees_ok(x_degree, y_degree)) { set_err("ripp_pc_srs_setup: x_degree + 1 must be a power of two (the second-tier argument halves it)"); return RIPP_ERR_ARG; }
    LOCK; ENGINE;
    const Fr a = load_fr(alpha), b = load_fr(beta);
    ripp_pc_srs* s = new ripp_pc_srs(); s->nx = x_degree + 1; s->ny = y_degree + 1;
    const G1A g = g1_generator(); const G2A h = g2_generator();
    s->g = to_jac(g); s->h = to_jac(h); s->g_beta = smul_host(g, b); s->h_alpha = smul_host(h, a);
    int32_t rc;
    if ((rc = s->powers.reserve(s->ny * sizeof(G1A))) || (rc = s->ip.hbp.reserve((2 * s->nx - 1) * sizeof(G2A))) ||
        (rc = pc_powers_dev<Fp>(e, g, a, s->ny, s->powers.as<G1A>())) || (rc = pc_powers_dev<Fp2>(e, h, b, 2 * s->nx - 1, s->ip.hbp.as<G2A>())) ||
        (rc = pc_srs_finish(e, s))) { pc_srs_free(s); return rc; }
    ++g_live_handles; *out = s; return RIPP_OK;
}
// the same from caller-supplied powers: kzg_powers[y_degree + 1] (affine), h_beta_powers[2 x_degree + 1] (projective, normalised on the device)
API int32_t ripp_pc_srs_create(const ripp_g1a* kzg_powers, size_t y_degree, const ripp_g2j* h_beta_powers, size_t x_degree, const ripp_g1j* g_beta, const ripp_g2j* h_alpha, ripp_pc_srs** out) {
    if (!kzg_powers || !h_beta_powers || !g_beta || !h_alpha || !out) return RIPP_ERR_ARG;
    if (!pc_degrees_ok(x_degree, y_degree)) { set_err("ripp_pc_srs_create: x_degree + 1 must be a power of two (the second-tier argument halves it)"); return RIPP_ERR_ARG; }
    LOCK; ENGINE;
    ripp_pc_srs* s = new ripp_pc_srs(); s->nx = x_degree + 1; s->ny = y_degree + 1;
    const size_t num = 2 * s->nx - 1;
    G1A g0; std::memcpy(&g0, kzg_powers, sizeof g0);
    s->g = to_jac(g0); s->h = load_jac<Fp2>(h_beta_powers); s->g_beta = load_jac<Fp>(g_beta); s->h_alpha = load_jac<Fp2>(h_alpha);
    int32_t rc; G2J* dj;
    if ((rc = s->powers.reserve(s->ny * sizeof(G1A))) || (rc = s->ip.hbp.reserve(num * sizeof(G2A)))) { pc_srs_free(s); return rc; }
    if (hipMemcpyAsync(s->powers.p, kzg_powers, s->ny * sizeof(G1A), hipMemcpyHostToDevice, e->stream) != hipSuccess) { pc_srs_free(s); set_err("ripp_pc_srs_create: hipMemcpyAsync failed"); return RIPP_ERR_DEVICE; }
    if ((rc = upload<G2J>(e, e->jacG2, h_beta_powers, num, &dj)) || (rc = e->normalize_dev<Fp2>(dj, num, s->ip.hbp.as<G2A>())) || (rc = pc_srs_finish(e, s))) { pc_srs_free(s); return rc; }
    ++g_live_handles; *out = s; return RIPP_OK;
}
API void ripp_pc_srs_destroy(ripp_pc_srs* s) { if (!s) return; LOCK; pc_srs_free(s); --g_live_handles; }
// parse_bivariate_degrees_from_srs (mod.rs:308-312)
API int32_t ripp_pc_srs_degrees(const ripp_pc_srs* s, size_t* x_degree, size_t* y_degree) {
    if (!s || !x_degree || !y_degree) return RIPP_ERR_ARG;
    *x_degree = s->nx - 1; *y_degree = s->ny - 1; return RIPP_OK;
}
// SRS::get_verifier_key (tipa/mod.rs:120-127)
API int32_t ripp_pc_srs_verifier_key(const ripp_pc_srs* s, ripp_verifier_srs* out) {
    if (!s || !out) return RIPP_ERR_ARG;
    std::memcpy(&out->g, &s->g, sizeof s->g); std::memcpy(&out->h, &s->h, sizeof s->h); std::memcpy(&out->g_beta, &s->g_beta, sizeof s->g_beta); std::memcpy(&out->h_alpha, &s->h_alpha, sizeof s->h_alpha);
    return RIPP_OK;
}
// the first-tier powers (kzg_srs of mod.rs:161-164), y_degree + 1 affine points
API int32_t ripp_pc_srs_kzg_powers(const ripp_pc_srs* s, ripp_g1a* out) {
    if (!s || !out) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    HIPCHK(hipMemcpyAsync(out, s->powers.p, s->ny * sizeof(G1A), hipMemcpyDeviceToHost, e->stream));
    return e->sync();
}

extern "C++" {
// rows x cols scalars of a host matrix with row pitch `stride` -> dense [rows][cols] in e->pc_coef (no padded copy on the host: a pitched copy)
static int32_t pc_upload_matrix(Engine* e, const ripp_fr* m, size_t rows, size_t cols, size_t stride, Fr** dev) {
    int32_t rc = e->pc_coef.reserve(std::max<size_t>(rows * cols, 1) * sizeof(Fr)); if (rc) return rc;
    if (rows && cols) HIPCHK(hipMemcpy2DAsync(e->pc_coef.p, cols * sizeof(Fr), m, stride * sizeof(Fr), cols * sizeof(Fr), rows, hipMemcpyHostToDevice, e->stream));
    *dev = e->pc_coef.as<Fr>(); return RIPP_OK;
}
// a flat coefficient array as the dense [rows][ny] matrix of its bivariate form (mod.rs:316-338), the tail of the last row zeroed ON THE DEVICE
static int32_t pc_upload_flat(Engine* e, const ripp_fr* c, size_t len, size_t ny, size_t* rows, Fr** dev) {
    *rows = (len + ny - 1) / ny;
    int32_t rc = e->pc_coef.reserve(std::max<size_t>(*rows * ny, 1) * sizeof(Fr)); if (rc) return rc;
    if (len) HIPCHK(hipMemcpyAsync(e->pc_coef.p, c, len * sizeof(Fr), hipMemcpyHostToDevice, e->stream));
    if (*rows * ny > len) HIPCHK(hipMemsetAsync(e->pc_coef.as<Fr>() + len, 0, (*rows * ny - len) * sizeof(Fr), e->stream));
    *dev = e->pc_coef.as<Fr>(); return RIPP_OK;
}
// DensePolynomial strips trailing zero coefficients (from_coefficients_vec): the length that counts
static size_t pc_stripped_len(const ripp_fr* c, size_t len) {
    while (len) { const uint64_t* l = c[len - 1].l; if (l[0] | l[1] | l[2] | l[3]) break; --len; }
    return len;
}
// quotient of p (m coefficients in device memory) by (X - z) into e->pc_q (m - 1 coefficients) and p(z): the suffix scan of msm_batch.hpp
static int32_t kzg_quotient_dev(Engine* e, const Fr* dp, size_t m, const Fr& z, Fr* eval_host) {
    if (m == 0) { *eval_host = Fr::zero(); return RIPP_OK; }
    const size_t nchunk = (m + KZG_CHUNK - 1) / KZG_CHUNK;
    int32_t rc;
    if ((rc = e->pc_h.reserve(nchunk * sizeof(Fr))) || (rc = e->pc_cin.reserve(nchunk * sizeof(Fr))) || (rc = e->pc_q.reserve((m + 1) * sizeof(Fr)))) return rc;
    Fr* const q = e->pc_q.as<Fr>();                                                    // q[0 .. m - 1), then one slot for p(z)
    kzg_quotient_launch(e->stream, dp, m, z, e->pc_h.as<Fr>(), e->pc_cin.as<Fr>(), q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(eval_host, q + m, sizeof(Fr), hipMemcpyDeviceToHost, e->stream));
    return e->sync();
}
// KZG::open (mod.rs:90-109) of a polynomial in device memory: proof = MSM(powers, quotient), eval = p(z)
static int32_t kzg_open_dev(Engine* e, const G1A* powers, const Fr* dp, size_t m, const Fr& z, G1J* proof, Fr* eval) {
    int32_t rc = kzg_quotient_dev(e, dp, m, z, eval); if (rc) return rc;
    *proof = jac_inf<Fp>();
    if (m < 2) return RIPP_OK;                                                        // a constant: the quotient is the zero polynomial
    return e->msm_dev<Fp>(powers, e->pc_q.as<Fr>(), m - 1, proof);
}
// e(com - g * eval, h) == e(proof, h_alpha - h * point)   (KZG::verify, mod.rs:111-119)
static int32_t kzg_verify_core(Engine* e, const VSrs& v, const G1J& com, const Fr& point, const Fr& eval, const G1J& proof, bool* ok) {
    const G1J l1 = add(com, neg(smul_host(to_affine(v.g), eval)));
    const G2J r2 = add(v.h_alpha, neg(smul_host(to_affine(v.h), point)));
    return pairing_eq(e, l1, v.h, proof, r2, ok);
}
}  // extern "C++"

// out[r] = sum_{i < cols} scalars[r * stride + i] * bases[i], r < rows: MultiexponentiationInnerProduct::inner_product (inner_products/src/lib.rs:128-141) of `rows`
// scalar vectors over ONE base vector, the y_polynomial_coms loop of mod.rs:188-193.  The bases are uploaded and extended once; bases [cols, n) take no part.
API int32_t ripp_msm_g1_batch_a(const ripp_g1a* bases, size_t n, const ripp_fr* scalars, size_t rows, size_t cols, size_t stride, ripp_g1j* out) {
    if (cols > n) { set_err("ripp_msm_g1_batch_a: cols = " + std::to_string(cols) + " exceeds the " + std::to_string(n) + " bases"); return RIPP_ERR_ARG; }
    if (stride < cols) { set_err("ripp_msm_g1_batch_a: stride = " + std::to_string(stride) + " is shorter than a row of " + std::to_string(cols)); return RIPP_ERR_ARG; }
    if (rows == 0) return RIPP_OK;
    if (!out || (cols && (!bases || !scalars)) || rows >= ((size_t)1 << 32) || cols >= ((size_t)1 << 30)) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    int32_t rc; G1A* db; Fr* ds;
    if ((rc = upload<G1A>(e, e->affG1, bases, cols, &db)) || (rc = pc_upload_matrix(e, scalars, rows, cols, stride, &ds)) || (rc = e->pc_out.reserve(rows * sizeof(G1J)))) return rc;
    if ((rc = e->msm_batch_dev<Fp>(db, nullptr, ds, rows, cols, cols, e->pc_out.as<G1J>()))) return rc;
    HIPCHK(hipMemcpyAsync(out, e->pc_out.p, rows * sizeof(G1J), hipMemcpyDeviceToHost, e->stream));
    return e->sync();
}
// chunks of rows the last batched MSM of this process ran in: 1 = one pass, more = ripp_config.mem_cap_bytes / free memory cut the batch, 0 = the per-row loop
// (legacy MSM switches, RIPP_NO_MSM_BATCH)
API int32_t ripp_msm_batch_chunks(void) { LOCK; return g_engine ? (int32_t)g_engine->msm_batch_chunks : 0; }

// KZG::commit (mod.rs:78-88)
API int32_t ripp_kzg_commit(const ripp_pc_srs* s, const ripp_fr* coeffs, size_t len, ripp_g1j* com) {
    if (!s || !com || (len && !coeffs)) return RIPP_ERR_ARG;
    len = pc_stripped_len(coeffs, len);
    if (len > s->ny) { set_err("ripp_kzg_commit: " + std::to_string(len) + " coefficients, " + std::to_string(s->ny) + " powers (assert at mod.rs:82)"); return RIPP_ERR_ARG; }
    LOCK; ENGINE;
    G1J res = jac_inf<Fp>(); int32_t rc; Fr* dc;
    if (len && ((rc = upload<Fr>(e, e->pc_coef, coeffs, len, &dc)) || (rc = e->msm_dev<Fp>(pc_key(s).bases, dc, len, &res)))) return rc;
    std::memcpy(com, &res, sizeof res); return RIPP_OK;
}
// KZG::open (mod.rs:90-109); eval (optional) = p(point), the remainder the reference drops
API int32_t ripp_kzg_open(const ripp_pc_srs* s, const ripp_fr* coeffs, size_t len, const ripp_fr* point, ripp_g1j* proof, ripp_fr* eval) {
    if (!s || !point || !proof || (len && !coeffs)) return RIPP_ERR_ARG;
    len = pc_stripped_len(coeffs, len);
    if (len > s->ny) { set_err("ripp_kzg_open: " + std::to_string(len) + " coefficients, " + std::to_string(s->ny) + " powers (assert at mod.rs:95)"); return RIPP_ERR_ARG; }
    LOCK; ENGINE;
    G1J pr; Fr ev; int32_t rc; Fr* dc;
    if ((rc = upload<Fr>(e, e->pc_coef, coeffs, len, &dc)) || (rc = kzg_open_dev(e, pc_key(s).bases, dc, len, load_fr(point), &pr, &ev))) return rc;
    std::memcpy(proof, &pr, sizeof pr); if (eval) std::memcpy(eval, &ev, sizeof ev);
    return RIPP_OK;
}
// KZG::verify (mod.rs:111-119)
API int32_t ripp_kzg_verify(const ripp_verifier_srs* v_srs, const ripp_g1j* com, const ripp_fr* point, const ripp_fr* eval, const ripp_g1j* proof, int32_t* accept) {
    if (!v_srs || !com || !point || !eval || !proof || !accept) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    bool ok = false; int32_t rc = kzg_verify_core(e, load_vsrs(v_srs), load_jac<Fp>(com), load_fr(point), load_fr(eval), load_jac<Fp>(proof), &ok); if (rc) return rc;
    *accept = ok ? 1 : 0; return RIPP_OK;
}

// BivariatePolynomialCommitment::commit (mod.rs:174-196): coeffs[i * stride + j] = coefficient j of y_polynomials[i], i < rows <= x_degree + 1 (missing rows are zero
// polynomials), j < cols <= y_degree + 1.  com = the AFGHO commitment to the x_degree + 1 KZG commitments y_coms.
API int32_t ripp_pc_commit(const ripp_pc_srs* s, const ripp_fr* coeffs, size_t rows, size_t cols, size_t stride, ripp_gt* com, ripp_g1j* y_coms) {
    if (!s || !com || !y_coms || (rows && cols && !coeffs) || stride < cols) return RIPP_ERR_ARG;
    int32_t rc; if ((rc = two_tier_fits("ripp_pc_commit", "the SRS degrees", pc_key(s), rows, cols))) return rc;
    LOCK; ENGINE;
    Fr* dc; if ((rc = pc_upload_matrix(e, coeffs, rows, cols, stride, &dc))) return rc;
    return two_tier_commit(e, pc_key(s), dc, rows, cols, cols, com, y_coms);
}

extern "C++" {
static bool pc_opening_ok(const ripp_pc_opening* o) { return o && o->com_gt && o->com_g1 && o->transcript; }
// BivariatePolynomialCommitment::open (mod.rs:198-263) on a dense coefficient matrix in device memory
static int32_t pc_open_dev(Engine* e, const ripp_pc_srs* s, const Fr* dcoef, size_t rows, size_t cols, size_t stride, const ripp_g1j* y_coms, const Fr& x, const Fr& y,
                           ripp_pc_opening* o, ripp_fr* eval, ripp_stats* st) {
    const TwoTier k = pc_key(s); int32_t rc;
    SsmVecs v; G1J yc, kp; Fr ev; double t_start;
    if ((rc = two_tier_open_prefix(e, k, v, dcoef, rows, cols, stride, x, &yc, &t_start, []() { return RIPP_OK; }))) return rc;          // y_eval_comm (mod.rs:236-240)
    if ((rc = kzg_open_dev(e, k.bases, e->pc_yev.as<Fr>(), k.ny, y, &kp, &ev))) return rc;                               // kzg_proof (mod.rs:252-256), p(x, y)
    // the second tier: TIPAWithSSM over (y_polynomial_comms, powers of x) under ck_1 (mod.rs:242-250)
    if ((rc = two_tier_load_second(e, k, v, y_coms))) return rc;
    G1A ha; Fr hs; G2A hka; G2J oa; Fr c;
    if ((rc = tipa_ssm_core(e, &s->ip, v, k.nx, o->com_gt, o->com_g1, o->transcript, ha, hs, hka, &oa, &c))) return rc;
    const G1J ja = to_jac(ha); const G2J jka = to_jac(hka);
    std::memcpy(&o->base_a, &ja, sizeof ja); std::memcpy(&o->base_b, &hs, sizeof hs); std::memcpy(&o->final_ck_a, &jka, sizeof jka); std::memcpy(&o->opening_a, &oa, sizeof oa);
    std::memcpy(&o->kzg_challenge, &c, sizeof c); std::memcpy(&o->y_eval_comm, &yc, sizeof yc); std::memcpy(&o->kzg_proof, &kp, sizeof kp);
    if (eval) std::memcpy(eval, &ev, sizeof ev);
    return finish_stats(e, t_start, st);
}
static int32_t pc_verify_core(Engine* e, const ripp_verifier_srs* v_srs, const ripp_gt* com, const Fr& x, const Fr& y, const Fr& eval, const ripp_pc_opening* o, size_t rounds, int32_t* accept) {
    int32_t ip_ok = 0; bool kzg_ok = false; int32_t rc;
    ripp_fr xs; std::memcpy(&xs, &x, sizeof xs);
    if ((rc = tipa_ssm_verify_core(e, v_srs, com, &o->y_eval_comm, &xs, o->com_gt, o->com_g1, rounds, &o->base_a, &o->final_ck_a, &o->opening_a, &ip_ok))) return rc;      // mod.rs:273-278
    if ((rc = kzg_verify_core(e, load_vsrs(v_srs), load_jac<Fp>(&o->y_eval_comm), y, eval, load_jac<Fp>(&o->kzg_proof), &kzg_ok))) return rc;                          // mod.rs:279-282
    *accept = (ip_ok && kzg_ok) ? 1 : 0; return RIPP_OK;
}
}  // extern "C++"

// BivariatePolynomialCommitment::open (mod.rs:198-263).  opening: caller-allocated step arrays for rounds = log2(x_degree + 1), filled in ROUND order like
// ripp_tipa_ssm_prove's; eval (optional) = p(x, y).  Needs x_degree >= 1.
API int32_t ripp_pc_open(const ripp_pc_srs* s, const ripp_fr* coeffs, size_t rows, size_t cols, size_t stride, const ripp_g1j* y_coms, const ripp_fr* x, const ripp_fr* y,
                         ripp_pc_opening* opening, ripp_fr* eval, ripp_stats* st) {
    if (!s || !y_coms || !x || !y || !pc_opening_ok(opening) || (rows && cols && !coeffs) || stride < cols) return RIPP_ERR_ARG;
    int32_t rc; if ((rc = two_tier_fits("ripp_pc_open", "the SRS degrees", pc_key(s), rows, cols))) return rc;
    if (s->nx < 2) return RIPP_ERR_POW2;
    LOCK; ENGINE;
    Fr* dc; if ((rc = pc_upload_matrix(e, coeffs, rows, cols, stride, &dc))) return rc;
    return pc_open_dev(e, s, dc, rows, cols, cols, y_coms, load_fr(x), load_fr(y), opening, eval, st);
}
// BivariatePolynomialCommitment::verify (mod.rs:265-285)
API int32_t ripp_pc_verify(const ripp_verifier_srs* v_srs, const ripp_gt* com, const ripp_fr* x, const ripp_fr* y, const ripp_fr* eval, const ripp_pc_opening* opening, size_t rounds, int32_t* accept) {
    if (!v_srs || !com || !x || !y || !eval || !pc_opening_ok(opening) || !accept || rounds == 0) return RIPP_ERR_ARG;
    LOCK; ENGINE;
    return pc_verify_core(e, v_srs, com, load_fr(x), load_fr(y), load_fr(eval), opening, rounds, accept);
}

// UnivariatePolynomialCommitment (mod.rs:298-388): the bivariate form of a flat coefficient array is that array with stride y_degree + 1 (mod.rs:316-338), the point
// is (z^(y_degree + 1), z).  len <= (x_degree + 1)(y_degree + 1) after the trailing zeros are stripped.
API int32_t ripp_pc_commit_univariate(const ripp_pc_srs* s, const ripp_fr* coeffs, size_t len, ripp_gt* com, ripp_g1j* y_coms) {
    if (!s || !com || !y_coms || (len && !coeffs)) return RIPP_ERR_ARG;
    len = pc_stripped_len(coeffs, len);
    int32_t rc; if ((rc = two_tier_flat_fits("ripp_pc_commit_univariate", "the SRS's", pc_key(s), len))) return rc;
    LOCK; ENGINE;
    Fr* dc; size_t rows; if ((rc = pc_upload_flat(e, coeffs, len, s->ny, &rows, &dc))) return rc;
    return two_tier_commit(e, pc_key(s), dc, rows, rows ? s->ny : 0, s->ny, com, y_coms);
}
API int32_t ripp_pc_open_univariate(const ripp_pc_srs* s, const ripp_fr* coeffs, size_t len, const ripp_g1j* y_coms, const ripp_fr* point, ripp_pc_opening* opening, ripp_fr* eval, ripp_stats* st) {
    if (!s || !y_coms || !point || !pc_opening_ok(opening) || (len && !coeffs)) return RIPP_ERR_ARG;
    len = pc_stripped_len(coeffs, len);
    int32_t rc; if ((rc = two_tier_flat_fits("ripp_pc_open_univariate", "the SRS's", pc_key(s), len))) return rc;
    if (s->nx < 2) return RIPP_ERR_POW2;
    LOCK; ENGINE;
    Fr* dc; size_t rows; if ((rc = pc_upload_flat(e, coeffs, len, s->ny, &rows, &dc))) return rc;
    const Fr z = load_fr(point);
    return pc_open_dev(e, s, dc, rows, rows ? s->ny : 0, s->ny, y_coms, fr_pow_u(z, s->ny), z, opening, eval, st);               // mod.rs:362-369
}
API int32_t ripp_pc_verify_univariate(const ripp_verifier_srs* v_srs, size_t max_degree, const ripp_gt* com, const ripp_fr* point, const ripp_fr* eval, const ripp_pc_opening* opening, size_t rounds, int32_t* accept) {
    if (!v_srs || !com || !point || !eval || !pc_opening_ok(opening) || !accept || rounds == 0) return RIPP_ERR_ARG;
    size_t xd, yd; int32_t rc = sqrt_split(max_degree, 16, "ripp_pc_univariate_degrees", "mod.rs:302-305", &xd, &yd); if (rc) return rc;
    LOCK; ENGINE;
    const Fr z = load_fr(point);
    return pc_verify_core(e, v_srs, com, fr_pow_u(z, yd + 1), z, load_fr(eval), opening, rounds, accept);                      // mod.rs:380-386
}
