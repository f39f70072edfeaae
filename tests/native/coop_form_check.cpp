// coop_form_check — prints the cooperative kernel form (csrc/rle_coop_limits.h) that sizes read from
// stdin select, one query per line (tests/test_coop_form.py):
//   enc MAX_LEN | dec MAX_IN_LEN MAX_OUT_LEN     ->  "W R" | "W UMAX R" | "none"
//   all                                          ->  every form the two functions return over the
//                                                    whole size range, one per line ("enc W R" /
//                                                    "dec W UMAX R"), each once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <tuple>

#include "rle_coop_limits.h"

// the selector is usable in constant expressions (the launchers may switch over it at compile time)
static_assert(rle::coop_enc_form(4097).W == 6 && rle::coop_dec_form(80640, 65536).R == 5, "constexpr");

int main() {
    char line[256];
    while (fgets(line, sizeof(line), stdin)) {
        char op[16];
        unsigned long long a = 0, b = 0;
        const int n = sscanf(line, "%15s %llu %llu", op, &a, &b);
        if (n < 1) continue;
        if (!strcmp(op, "enc") && n == 2) {
            const rle::CoopEncForm f = rle::coop_enc_form(a);
            if (f.W) printf("%u %u\n", f.W, f.R);
            else printf("none\n");
        } else if (!strcmp(op, "dec") && n == 3) {
            const rle::CoopDecForm f = rle::coop_dec_form(a, b);
            if (f.W) printf("%u %u %u\n", f.W, f.Umax, f.R);
            else printf("none\n");
        } else if (!strcmp(op, "all") && n == 1) {
            // every input length; for decode every stream length against every output length that is a
            // band edge or next to one, and a few inside the bands
            std::set<std::tuple<unsigned, unsigned>> enc;
            for (unsigned long long u = 0; u <= rle::kCoopEncMaxBytes + 2048; ++u) {
                const rle::CoopEncForm f = rle::coop_enc_form(u);
                if (f.W) enc.insert({f.W, f.R});
            }
            for (const auto& e : enc) printf("enc %u %u\n", std::get<0>(e), std::get<1>(e));
            std::set<std::tuple<unsigned, unsigned, unsigned>> dec;
            std::set<unsigned long long> us;
            for (unsigned long long m = 0; m <= rle::kCoopDecUmax + 4096; m += 4096) {
                us.insert(m ? m - 1 : 0);
                us.insert(m);
                us.insert(m + 1);
                for (unsigned long long u = m + 341; u < m + 4096; u += 341) us.insert(u);
            }
            for (const unsigned long long u : us)
                for (unsigned long long c = 0; c <= rle::kCoopDecMaxIn + 2016; ++c) {
                    const rle::CoopDecForm f = rle::coop_dec_form(c, u);
                    if (f.W) dec.insert({f.W, f.Umax, f.R});
                }
            for (const auto& d : dec) printf("dec %u %u %u\n", std::get<0>(d), std::get<1>(d), std::get<2>(d));
        } else {
            return 2;
        }
    }
    return 0;
}
