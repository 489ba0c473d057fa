// Stand-alone driver of the Blake2b challenges of ripp_amd/csrc/host_fs.hpp (tests/test_fs_challenges_cpu.py builds and runs it; no device, no library).
// Prints one line per case: name, the challenge, and for the GIPA kinds c_inv, as hex of the canonical integers.
//
// Inputs (the test's model rebuilds them): a splitmix64 stream, one field element = BITS / 64 (rounded up) draws read little-endian and cut to
// BITS - 1 bits, hence below the modulus; members are drawn coordinate by coordinate in the order of their byte image's natural form
// (Fp2 = c0, c1; point = x, y; Fp12 = c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2), a round's members in the order l1, r1, t1, l2, r2, t2.
// Members need not be on the curve or in GT: only their byte image is hashed.  Variants of every GIPA kind:
//   first  no previous challenge                      later  a drawn previous challenge
//   edge   previous challenge r - 1; com_1 holds the point at infinity, Fr 0 and a GT value starting 0, 1, p - 1; com_2 coordinates p - 1, 1, Fr r - 1
//   sign   previous challenge 1; com_2 = com_1 with every point negated (y and -y straddle the BLS12-377 sign flag)
//   sign0  the same with y.c1 = 0 in G2 (the flag then compares y.c0)
#include "host_fs.hpp"
#include <cstdio>

using namespace ripp;

static uint64_t g_state = 0x5eed0001ull;
static uint64_t next64() {
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
template <class P> static Mont<P> draw() {
    Mont<P> t;
    for (int i = 0; i < P::N / 2; ++i) { const uint64_t u = next64(); t.l[2 * i] = (uint32_t)u; t.l[2 * i + 1] = (uint32_t)(u >> 32); }
    const int keep = P::BITS - 1;
    for (int i = 0; i < P::N; ++i) { const int b = keep - 32 * i; if (b <= 0) t.l[i] = 0; else if (b < 32) t.l[i] &= (1u << b) - 1u; }
    return to_mont(t);
}
static Fp fp() { return draw<FpParams>(); }
static Fr fr() { return draw<FrParams>(); }
static const Fp P0 = Fp::zero(), P1 = Fp::one(), PM = neg(Fp::one());

enum Variant { FIRST, LATER, EDGE, SIGN, SIGN0 };
// one member of side j (0: com_1, 1: com_2) for a variant; `twin` is com_1's member when j = 1
static void member(Fp12& x, Variant v, int j, const Fp12& twin) {
    Fp* c[12] = {&x.c0.c0.c0, &x.c0.c0.c1, &x.c0.c1.c0, &x.c0.c1.c1, &x.c0.c2.c0, &x.c0.c2.c1, &x.c1.c0.c0, &x.c1.c0.c1, &x.c1.c1.c0, &x.c1.c1.c1, &x.c1.c2.c0, &x.c1.c2.c1};
    if (v == EDGE && j == 1) { for (Fp* p : c) *p = PM; return; }
    if (v >= SIGN && j == 1) { x = twin; return; }
    for (Fp* p : c) *p = fp();
    if (v == EDGE) { *c[0] = P0; *c[1] = P1; *c[2] = PM; }
}
static void member(G1A& x, Variant v, int j, const G1A& twin) {
    if (v == EDGE) { x = j ? G1A{PM, P1} : G1A{P0, P0}; return; }
    if (v >= SIGN && j == 1) { x = neg(twin); return; }
    x.x = fp(); x.y = fp();
}
static void member(G2A& x, Variant v, int j, const G2A& twin) {
    if (v == EDGE) { x = j ? G2A{{PM, P0}, {P1, PM}} : G2A{{P0, P0}, {P0, P0}}; return; }
    if (v >= SIGN && j == 1) { x = neg(twin); return; }
    x.x.c0 = fp(); x.x.c1 = fp(); x.y.c0 = fp(); x.y.c1 = fp();
    if (v == SIGN0) x.y.c1 = P0;
}
static void member(Fr& x, Variant v, int j, const Fr& twin) {
    if (v == EDGE) { x = j ? neg(Fr::one()) : Fr::zero(); return; }
    if (v >= SIGN && j == 1) { x = twin; return; }
    x = fr();
}
static void member(fs::SSMPlaceholder&, Variant, int, const fs::SSMPlaceholder&) {}

static void print_fr(const Fr& a) { const Fr c = from_mont(a); printf(" 0x"); for (int i = 7; i >= 0; --i) printf("%08x", c.l[i]); }

template <class L, class R, class T> static void gipa_kind(const char* kind) {
    static const char* names[] = {"first", "later", "edge", "sign", "sign0"};
    for (int vi = 0; vi < 5; ++vi) {
        const Variant v = (Variant)vi;
        Fr prev = Fr::zero();
        if (v == LATER) prev = fr(); else if (v == EDGE) prev = neg(Fr::one()); else if (v >= SIGN) prev = Fr::one();
        fs::Com<L, R, T> s[2];
        for (int j = 0; j < 2; ++j) { member(s[j].l, v, j, s[0].l); member(s[j].r, v, j, s[0].r); member(s[j].t, v, j, s[0].t); }
        Fr c_inv; const Fr c = fs::gipa_challenge(v == FIRST ? nullptr : &prev, s[0], s[1], c_inv);
        printf("%s_%s", kind, names[vi]); print_fr(c); print_fr(c_inv); printf("\n");
    }
}
static void line(const char* name, const Fr& c) { printf("%s", name); print_fr(c); printf("\n"); }

int main() {
    gipa_kind<Fp12, Fp12, Fp12>("tipp");
    gipa_kind<Fp12, fs::SSMPlaceholder, G1A>("ssm");
    gipa_kind<Fp12, G1A, G1A>("mexp");
    gipa_kind<G2A, G1A, Fr>("scalar");
    gipa_kind<G1A, fs::SSMPlaceholder, Fr>("scalar_ssm");

    Fr first = fr(); G2A ka; G1A kb; member(ka, FIRST, 0, ka); member(kb, FIRST, 0, kb);
    line("kzg_ab", fs::kzg_challenge(first, ka, &kb));
    line("kzg_a", fs::kzg_challenge(first, ka, nullptr));
    const G2A ka_n = neg(ka); const G1A kb_n = neg(kb);
    line("kzg_sign_ab", fs::kzg_challenge(Fr::one(), ka_n, &kb_n));
    member(ka, EDGE, 0, ka); member(kb, EDGE, 0, kb);
    line("kzg_edge_ab", fs::kzg_challenge(neg(Fr::one()), ka, &kb));
    member(ka, EDGE, 1, ka);
    line("kzg_edge_a", fs::kzg_challenge(Fr::zero(), ka, nullptr));

    Fp12 g[3]; for (Fp12& x : g) member(x, FIRST, 0, x);
    line("agg", fs::aggregation_challenge(g[0], g[1], g[2]));
    member(g[0], EDGE, 0, g[0]); member(g[1], EDGE, 1, g[1]);
    line("agg_edge", fs::aggregation_challenge(g[0], g[1], g[2]));
    return 0;
}
