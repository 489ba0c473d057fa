// Included by engine.hip inside its `extern "C"` block (after vec_api.inc: ripp_vec_validate reads resident vectors and views in place).
// ---- validation of untrusted points (fq_validate.hpp) -------------------------------------------------------------------------------------------
// Host slices go through the engine's affine scratch (affG1 / affG2) in chunks of g_validate_chunk points; the flag bytes of a chunk come back through
// fix_flags and n_bad / first_bad are counted on the host.  The byte readers parse on the host workers with wire.hpp's parse_g1 / parse_g2 (flags, range,
// curve equation, square roots -- the code the single-element readers run) and send only the parsed points to the device for the subgroup test.
// The host parse of chunk k + 1 does NOT overlap the device check of chunk k: a chunk is parsed, checked, and then the next one starts.
extern "C++" {
static constexpr size_t VALIDATE_CHUNK_DEFAULT = (size_t)1 << 20;
static size_t g_validate_chunk = VALIDATE_CHUNK_DEFAULT;          // points per launch (ripp_validate_set_chunk: tests place chunk seams at small n)
// flags of m <= 2^31 points that are ALREADY on the device -> host_flags[m]
template <class F> static int32_t validate_dev(Engine* e, const Affine<F>* dp, size_t m, uint8_t* host_flags) {
    int32_t rc = e->fix_flags.reserve((m + 15) / 16 * 16 + 16); if (rc) return rc;
    uint8_t* df = e->fix_flags.as<uint8_t>();
    const ValDigits dg = val_digits((const F*)nullptr);
    if constexpr (std::is_same<F, Fp>::value) {
        hipLaunchKernelGGL(k_validate_g1_q, dim3(nblk(m, 256)), dim3(256), 0, e->stream, dp, (uint32_t)m, dg, df);
    } else {
        hipLaunchKernelGGL(k_validate_g2_q, dim3(nblk(m, 64)), dim3(64), 0, e->stream, dp, (uint32_t)m, dg, df);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_validate_fix<Fp2>), dim3(std::min<unsigned>(FIX_GRID, nblk((m + 15) / 16, 64))), dim3(64), 0, e->stream, dp, (uint32_t)m, dg, df);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(host_flags, df, m, hipMemcpyDeviceToHost, e->stream));
    return e->sync();
}
static size_t validate_chunk_len() { return std::min<size_t>(std::max<size_t>(g_validate_chunk, 1), (size_t)1 << 30); }
// a vector on the device (a resident vector or view), chunk by chunk
template <class F> static int32_t validate_resident(Engine* e, const Affine<F>* dp, size_t n, uint8_t* flags) {
    const size_t chunk = validate_chunk_len();
    for (size_t off = 0; off < n; off += chunk) { const int32_t rc = validate_dev<F>(e, dp + off, std::min(chunk, n - off), flags + off); if (rc) return rc; }
    return RIPP_OK;
}
// a host slice: each chunk uploaded into the engine's affine scratch
template <class F> static int32_t validate_host(Engine* e, const Affine<F>* hp, size_t n, uint8_t* flags) {
    const size_t chunk = validate_chunk_len();
    DevBuf& buf = std::is_same<F, Fp>::value ? e->affG1 : e->affG2;
    for (size_t off = 0; off < n; off += chunk) {
        const size_t m = std::min(chunk, n - off);
        Affine<F>* dp; int32_t rc = upload<Affine<F>>(e, buf, hp + off, m, &dp); if (rc) return rc;
        if ((rc = validate_dev<F>(e, dp, m, flags + off))) return rc;
    }
    return RIPP_OK;
}
// `group` consecutive flag bytes make one item (a point, or the three points of a proof)
static void validate_count(const uint8_t* flags, size_t n, size_t group, size_t* n_bad, size_t* first_bad) {
    size_t bad = 0, first = n;
    for (size_t i = 0; i < n; ++i) {
        bool b = false; for (size_t k = 0; k < group; ++k) b |= flags[i * group + k] != 0;
        if (b) { if (!bad) first = i; ++bad; }
    }
    *n_bad = bad; *first_bad = first;
}
template <class F> static int32_t validate_slice_api(const void* p, size_t n, uint8_t* flags, size_t* n_bad, size_t* first_bad) {
    if (!p || !n_bad || !first_bad) return RIPP_ERR_ARG;
    if (n == 0) { *n_bad = 0; *first_bad = 0; return RIPP_OK; }
    LOCK; ENGINE;
    std::vector<uint8_t> own; if (!flags) { own.resize(n); flags = own.data(); }
    const int32_t rc = validate_host<F>(e, static_cast<const Affine<F>*>(p), n, flags); if (rc) return rc;
    validate_count(flags, n, 1, n_bad, first_bad); return RIPP_OK;
}
static inline int parse_pt(const uint8_t* in, bool c, G1A& p) { return wire::parse_g1(in, c, p); }
static inline int parse_pt(const uint8_t* in, bool c, G2A& p) { return wire::parse_g2(in, c, p); }
// images [lo, hi) of a strided array -> out / flags (the same stride in points and flag bytes for both outputs: 1 for a vector, 3 for the proofs' flags)
template <class F> static void parse_range(const uint8_t* in, size_t stride, bool c, size_t lo, size_t hi, Affine<F>* out, uint8_t* flags, size_t fstride) {
    for (size_t i = lo; i < hi; ++i) {
        Affine<F> p; const int f = parse_pt(in + i * stride, c, p);
        out[i] = f ? aff_inf<F>() : p; flags[i * fstride] = (uint8_t)f;
    }
}
// fn(lo, hi) over [0, n) on the host workers and the caller's thread
template <class FN> static void validate_parallel(size_t n, FN&& fn) {
    const size_t parts = std::min<size_t>(n, (size_t)host_pool().size() + 1);
    if (parts <= 1) { fn((size_t)0, n); return; }
    host_pool().parallel((int)parts, [&](int t) { fn(n * (size_t)t / parts, n * ((size_t)t + 1) / parts); });
}
// device flags of a parsed chunk folded into the parse flags: a point that parsed and fails on the device is outside the subgroup
template <class F> static void validate_merge(const uint8_t* dev, size_t m, Affine<F>* out, uint8_t* flags, size_t fstride) {
    for (size_t i = 0; i < m; ++i) if (!flags[i * fstride] && dev[i]) { flags[i * fstride] = dev[i]; out[i] = aff_inf<F>(); }
}
template <class F> static int32_t de_vec_api(const uint8_t* in, size_t stride, size_t n, int32_t compress, Affine<F>* out, uint8_t* flags, size_t* n_bad, size_t* first_bad) {
    const bool c = compress != 0;
    const size_t size = std::is_same<F, Fp>::value ? wire::g1_size(c) : wire::g2_size(c);
    if (!in || !out || !n_bad || !first_bad || stride < size) return RIPP_ERR_ARG;
    if (n == 0) { *n_bad = 0; *first_bad = 0; return RIPP_OK; }
    LOCK; ENGINE;
    std::vector<uint8_t> own; if (!flags) { own.resize(n); flags = own.data(); }
    const size_t chunk = validate_chunk_len();
    std::vector<uint8_t> dev(std::min(chunk, n));
    DevBuf& buf = std::is_same<F, Fp>::value ? e->affG1 : e->affG2;
    double parse_ms = 0, check_ms = 0;
    for (size_t off = 0; off < n; off += chunk) {
        const size_t m = std::min(chunk, n - off);
        const double t0 = now_ms();
        validate_parallel(m, [&](size_t lo, size_t hi) { parse_range<F>(in + off * stride, stride, c, lo, hi, out + off, flags + off, 1); });
        const double t1 = now_ms();
        Affine<F>* dp; int32_t rc = upload<Affine<F>>(e, buf, out + off, m, &dp); if (rc) return rc;
        if ((rc = validate_dev<F>(e, dp, m, dev.data()))) return rc;
        validate_merge<F>(dev.data(), m, out + off, flags + off, 1);
        parse_ms += t1 - t0; check_ms += now_ms() - t1;
    }
    if (trace_on()) fprintf(stderr, "[ripp] de_vec(%zu, compress %d): host parse %.3f ms, device check %.3f ms\n", n, (int)c, parse_ms, check_ms);
    validate_count(flags, n, 1, n_bad, first_bad); return RIPP_OK;
}
}  // extern "C++"

API int32_t ripp_validate_g1a(const ripp_g1a* p, size_t n, uint8_t* flags, size_t* n_bad, size_t* first_bad) { return validate_slice_api<Fp>(p, n, flags, n_bad, first_bad); }
API int32_t ripp_validate_g2a(const ripp_g2a* p, size_t n, uint8_t* flags, size_t* n_bad, size_t* first_bad) { return validate_slice_api<Fp2>(p, n, flags, n_bad, first_bad); }
API int32_t ripp_vec_validate(const ripp_vec* v, uint8_t* flags, size_t* n_bad, size_t* first_bad) {
    if (!v || !n_bad || !first_bad || (v->kind != RIPP_VEC_G1 && v->kind != RIPP_VEC_G2)) return RIPP_ERR_ARG;
    if (v->len == 0) { *n_bad = 0; *first_bad = 0; return RIPP_OK; }
    LOCK; ENGINE;
    std::vector<uint8_t> own; if (!flags) { own.resize(v->len); flags = own.data(); }
    const int32_t rc = v->kind == RIPP_VEC_G1 ? validate_resident<Fp>(e, vec_ptr<G1A>(v), v->len, flags) : validate_resident<Fp2>(e, vec_ptr<G2A>(v), v->len, flags);
    if (rc) return rc;
    validate_count(flags, v->len, 1, n_bad, first_bad); return RIPP_OK;
}
API int32_t ripp_de_g1_vec(const uint8_t* in, size_t stride, size_t n, int32_t compress, ripp_g1a* out, uint8_t* flags, size_t* n_bad, size_t* first_bad) {
    return de_vec_api<Fp>(in, stride, n, compress, reinterpret_cast<G1A*>(out), flags, n_bad, first_bad);
}
API int32_t ripp_de_g2_vec(const uint8_t* in, size_t stride, size_t n, int32_t compress, ripp_g2a* out, uint8_t* flags, size_t* n_bad, size_t* first_bad) {
    return de_vec_api<Fp2>(in, stride, n, compress, reinterpret_cast<G2A*>(out), flags, n_bad, first_bad);
}
// n ark_groth16::Proof images (A, B, C).  Per chunk of proofs: parse, then ONE G1 launch over A | C and one G2 launch over B.
API int32_t ripp_de_groth16_proofs(const uint8_t* in, size_t stride, size_t n, int32_t compress, ripp_g1a* a, ripp_g2a* b, ripp_g1a* c,
                                   uint8_t* flags, size_t* n_bad, size_t* first_bad) {
    const bool cz = compress != 0;
    const size_t s1 = wire::g1_size(cz), s2 = wire::g2_size(cz);
    if (!in || !a || !b || !c || !n_bad || !first_bad || stride < 2 * s1 + s2) return RIPP_ERR_ARG;
    if (n == 0) { *n_bad = 0; *first_bad = 0; return RIPP_OK; }
    LOCK; ENGINE;
    G1A* pa = reinterpret_cast<G1A*>(a); G2A* pb = reinterpret_cast<G2A*>(b); G1A* pc = reinterpret_cast<G1A*>(c);
    std::vector<uint8_t> own; if (!flags) { own.resize(3 * n); flags = own.data(); }
    const size_t chunk = std::max<size_t>(validate_chunk_len() / 2, 1);       // proofs per chunk: A | C fill one G1 launch of the chunk length
    std::vector<uint8_t> dev(2 * std::min(chunk, n));
    double parse_ms = 0, check_ms = 0;
    for (size_t off = 0; off < n; off += chunk) {
        const size_t m = std::min(chunk, n - off);
        const uint8_t* img = in + off * stride; uint8_t* fl = flags + 3 * off;
        const double t0 = now_ms();
        validate_parallel(m, [&](size_t lo, size_t hi) {
            parse_range<Fp>(img, stride, cz, lo, hi, pa + off, fl, 3);
            parse_range<Fp2>(img + s1, stride, cz, lo, hi, pb + off, fl + 1, 3);
            parse_range<Fp>(img + s1 + s2, stride, cz, lo, hi, pc + off, fl + 2, 3);
        });
        const double t1 = now_ms();
        int32_t rc = e->affG1.reserve(2 * m * sizeof(G1A)); if (rc) return rc;
        G1A* d1 = e->affG1.as<G1A>();
        HIPCHK(hipMemcpyAsync(d1, pa + off, m * sizeof(G1A), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(d1 + m, pc + off, m * sizeof(G1A), hipMemcpyHostToDevice, e->stream));
        if ((rc = validate_dev<Fp>(e, d1, 2 * m, dev.data()))) return rc;
        validate_merge<Fp>(dev.data(), m, pa + off, fl, 3); validate_merge<Fp>(dev.data() + m, m, pc + off, fl + 2, 3);
        G2A* d2; if ((rc = upload<G2A>(e, e->affG2, pb + off, m, &d2))) return rc;
        if ((rc = validate_dev<Fp2>(e, d2, m, dev.data()))) return rc;
        validate_merge<Fp2>(dev.data(), m, pb + off, fl + 1, 3);
        parse_ms += t1 - t0; check_ms += now_ms() - t1;
    }
    if (trace_on()) fprintf(stderr, "[ripp] de_groth16_proofs(%zu, compress %d): host parse %.3f ms, device check %.3f ms\n", n, (int)cz, parse_ms, check_ms);
    validate_count(flags, n, 3, n_bad, first_bad); return RIPP_OK;
}
// Test hook: points per device launch of the calls above (0 restores the default, 2^20); returns the previous value.  Not a tuning knob -- it exists so
// that a test can put chunk seams into a vector of a few hundred points.
API size_t ripp_validate_set_chunk(size_t chunk) { LOCK; const size_t old = g_validate_chunk; g_validate_chunk = chunk ? chunk : VALIDATE_CHUNK_DEFAULT; return old; }
