// Stand-alone driver of the host side of point validation (tests/test_validate_inputs_cpu.py builds it per curve, also under AddressSanitizer + UBSan;
// no device, no library): val_complete of ripp_amd/csrc/fq_validate.hpp -- the check the device kernels redo their exceptional lanes with, and the same
// criterion their fast chains evaluate -- beside the DEFINITION (range, curve equation, [r]P = O by plain double-and-add), and the parse / subgroup
// split of wire.hpp beside the single-element readers built from it.
//
// stdin, one request per line (hex without prefix):
//   1 <x> <y>                  a G1 point: the 384-bit MONTGOMERY limb values as they lie in memory (may be >= p)
//   2 <x0> <x1> <y0> <y1>      a G2 point
//   W <g> <c> <bytes>          an ark-serialize image of group g (1 / 2), compress c (0 / 1)
// stdout, one line per request:  "<val_complete flag> <definition flag>"  or  "<parse result> <1 when get_g accepts>".
#include "fq_validate.hpp"
#include "wire.hpp"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

using namespace ripp;

static int hexv(char ch) { return ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : ch >= 'A' && ch <= 'F' ? ch - 'A' + 10 : -1; }
static Fp limbs(const std::string& hex) {
    Fp c = Fp::zero();
    const int n = (int)hex.size();
    if (n == 0 || n > 96) { fprintf(stderr, "bad field element\n"); exit(2); }
    for (int i = 0; i < n; ++i) { const int v = hexv(hex[n - 1 - i]); if (v < 0) { fprintf(stderr, "bad hex digit\n"); exit(2); } c.l[i / 8] |= (uint32_t)v << (4 * (i % 8)); }
    return c;
}
template <class F> static int by_definition(const Affine<F>& p) {
    if (!val_reduced(p.x) || !val_reduced(p.y)) return 1;
    if (is_inf(p)) return 0;
    if (!wire::on_curve(p)) return 2;
    return wire::in_subgroup(p) ? 0 : 3;
}

int main() {
    const ValDigits d1 = val_digits((const Fp*)nullptr), d2 = val_digits((const Fp2*)nullptr);
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream is(line);
        std::string tag; is >> tag;
        if (tag == "1") {
            std::string x, y; is >> x >> y;
            const G1A p{limbs(x), limbs(y)};
            printf("%d %d\n", (int)val_complete<Fp>(p, d1), by_definition(p));
        } else if (tag == "2") {
            std::string x0, x1, y0, y1; is >> x0 >> x1 >> y0 >> y1;
            const G2A p{{limbs(x0), limbs(x1)}, {limbs(y0), limbs(y1)}};
            printf("%d %d\n", (int)val_complete<Fp2>(p, d2), by_definition(p));
        } else if (tag == "W") {
            int g, c; std::string hex; is >> g >> c >> hex;
            const size_t size = g == 1 ? wire::g1_size(c != 0) : wire::g2_size(c != 0);
            if (hex.size() != 2 * size) { fprintf(stderr, "bad image length\n"); return 2; }
            std::string raw(size, '\0');
            for (size_t i = 0; i < size; ++i) raw[i] = (char)(hexv(hex[2 * i]) * 16 + hexv(hex[2 * i + 1]));
            const uint8_t* in = reinterpret_cast<const uint8_t*>(raw.data());
            if (g == 1) { G1A p, q; const int r = wire::parse_g1(in, c != 0, p); printf("%d %d\n", r, (int)wire::get_g1(in, c != 0, q)); }
            else { G2A p, q; const int r = wire::parse_g2(in, c != 0, p); printf("%d %d\n", r, (int)wire::get_g2(in, c != 0, q)); }
        } else { fprintf(stderr, "bad request: %s\n", line.c_str()); return 2; }
    }
    return 0;
}
