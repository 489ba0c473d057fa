// Stand-alone driver of the host scalar recoders of ripp_amd/csrc/recode.hpp (tests/test_recoders_cpu.py builds and runs it per curve; no device, no library).
//
// stdin, one request per line (canonical integers below r, hex without prefix):
//   S <s>            every one-scalar recoder on s
//   P <x0> <x1>      the fused recoders on the pair (both below 2^128)
// stdout: the request line echoed, then one line per recoder:  <tag> <len> <string 0> <string 1> ...
// Every string is printed over the struct's FULL capacity (not just len), one character per digit: chr('P' + d) for -32 <= d < 32, '?' otherwise.
// Tags ending in .W are run for the two wNAF widths the engine uses, W = tab_width(4) and tab_width(FOLD_TAB_M); the first line printed is "W <w1> <w2>".
// The recoders that take 128-bit challenges only (split32_wnaf, split64_digits, split_digits_g1) are run iff fits_128 holds, as in the engine.
#include "recode.hpp"
#include <cstdio>
#include <cstdlib>

using namespace ripp;

static Fr parse(const char* hex) {
    Fr c = Fr::zero();
    int n = 0; while (hex[n] && hex[n] != '\n' && hex[n] != ' ') ++n;
    if (n == 0 || n > 64) { fprintf(stderr, "bad scalar\n"); exit(2); }
    for (int i = 0; i < n; ++i) {
        const char ch = hex[n - 1 - i];
        const int v = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : ch >= 'A' && ch <= 'F' ? ch - 'A' + 10 : -1;
        if (v < 0) { fprintf(stderr, "bad hex digit\n"); exit(2); }
        c.l[i / 8] |= (uint32_t)v << (4 * (i % 8));
    }
    return to_mont(c);
}
// nstr strings of cap digits each, contiguous
static void emit(const char* tag, int W, const int8_t* d, int nstr, int cap, int len) {
    if (W) printf("%s.%d %d", tag, W, len); else printf("%s %d", tag, len);
    for (int s = 0; s < nstr; ++s) {
        putchar(' ');
        for (int i = 0; i < cap; ++i) { const int v = d[s * cap + i]; putchar(v >= -32 && v < 32 ? 'P' + v : '?'); }
    }
    putchar('\n');
}
template <class T, int NSTR, int CAP> static void emit(const char* tag, int W, const int8_t (&d)[NSTR][CAP], const T& g) {
    static_assert(sizeof(T) >= NSTR * CAP, "layout"); emit(tag, W, &d[0][0], NSTR, CAP, g.len);
}

static void one_scalar(const Fr& s, const int W[2]) {
    const ScalarBits sb = scalar_bits(s);
    printf("scalar_bits %d", sb.nbits); for (int i = 7; i >= 0; --i) printf("%s%08x", i == 7 ? " " : "", sb.w[i]); printf("\n");
    const bool f128 = fits_128(s);
    printf("fits_128 %d\n", (int)f128);
    { const NafDigits g = naf_digits(s); emit("naf_digits", 0, g.d, 1, 260, g.len); }
    { const GlsDigits g = gls_digits(s); emit("gls_digits", 0, g.d, g); }
    { uint32_t rem[9], quo[8]; glv_split(s, rem, quo);
      printf("glv_split"); for (int i = 8; i >= 0; --i) printf("%s%08x", i == 8 ? " " : "", rem[i]); for (int i = 7; i >= 0; --i) printf("%s%08x", i == 7 ? " " : "", quo[i]); printf("\n"); }
    { const GlvDigits g = glv_digits(s); int8_t d[2][132]; std::memcpy(d[0], g.d1, 132); std::memcpy(d[1], g.d2, 132); emit("glv_digits", 0, d, g); }
    { const Gls8Digits g = gls8_digits(s); emit("gls8_digits", 0, g.d, g); }
    { const SplitDigits g = split_digits_g2(s); emit("split_digits_g2", 0, g.d, g); }
    { const SplitDigits g = split_digits_g1_glv(s); emit("split_digits_g1_glv", 0, g.d, g); }
    if (f128) {
        { const GlvDigits g = split64_digits(s); int8_t d[2][132]; std::memcpy(d[0], g.d1, 132); std::memcpy(d[1], g.d2, 132); emit("split64_digits", 0, d, g); }
        { const SplitDigits g = split_digits_g1(s); emit("split_digits_g1", 0, g.d, g); }
    }
    const Fr c = from_mont(s);
    const uint64_t low = (uint64_t)c.l[0] | ((uint64_t)c.l[1] << 32);
    for (int k = 0; k < 2; ++k) {
        const int w = W[k];
        { int8_t d[68]; std::memset(d, 0, sizeof d); const int len = wnaf4_recode(low, d, 66, w); emit("wnaf4_recode", w, d, 1, 68, len); }
        { const Wnaf16 g = gls16_wnaf(s, w); emit("gls16_wnaf", w, g.d, g); }
        { const GlsDigits g = gls_wnaf(s, w); emit("gls_wnaf", w, g.d, g); }
        if (f128) { const Wnaf4 g = split32_wnaf(s, w); emit("split32_wnaf", w, g.d, g); }
    }
}
static void pair(const Fr& x0, const Fr& x1, const int W[2]) {
    if (!fits_128(x0) || !fits_128(x1)) { fprintf(stderr, "fused recoders take 128-bit challenges\n"); exit(2); }
    for (int k = 0; k < 2; ++k) {
        const int w = W[k];
        { const WnafG1x4 g = fused_digits_g1(x0, x1, w); emit("fused_digits_g1", w, g.d, g); }
        { const Wnaf16x3 g = fused_digits_g2(x0, x1, w);
          int8_t d[48][20]; for (int t = 0; t < 3; ++t) std::memcpy(d[16 * t], g.s[t].d, sizeof g.s[t].d);
          printf("fused_digits_g2_lens.%d %d %d %d\n", w, g.s[0].len, g.s[1].len, g.s[2].len);
          emit("fused_digits_g2", w, d, g); }
    }
}

int main() {
    const int W[2] = {tab_width(4), tab_width(FOLD_TAB_M)};
    printf("W %d %d\n", W[0], W[1]);
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        if (line[0] == '\n' || line[0] == 0) continue;
        fputs(line, stdout);
        if (line[0] == 'S' && line[1] == ' ') one_scalar(parse(line + 2), W);
        else if (line[0] == 'P' && line[1] == ' ') {
            const char* sp = std::strchr(line + 2, ' ');
            if (!sp) { fprintf(stderr, "P takes two scalars\n"); return 2; }
            pair(parse(line + 2), parse(sp + 1), W);
        } else { fprintf(stderr, "unknown request\n"); return 2; }
    }
    return 0;
}
