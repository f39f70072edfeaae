// route_check — prints the drop-in's route (csrc/rle_route.h) for sizes and settings read from stdin,
// one query per line (tests/test_route.py):
//   [zerocopy=0|1] [zc_seg=N] [zc_coop=0|1] [reg_min=N] [fake_devs=N] then
//   compress U | decompress C U E | append C U A MAX_WHOLE MAX_TAIL | readn C U
// (MAX_WHOLE / MAX_TAIL: rle_max_compressed_size(U + A) / (16 + A), which the library defines).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rle_route.h"

static const char* body_name(rle::Body b) {
    switch (b) {
    case rle::Body::MappedOne: return "mapped_one";
    case rle::Body::MappedSeg: return "mapped_seg";
    case rle::Body::Staged: return "staged";
    case rle::Body::Large: return "large";
    }
    return "?";
}
static void print_call(const rle::CallRoute& r) {
    printf("reg=%d body=%s dev_seg=%d one_trip=%d\n", (int)r.reg, body_name(r.body), (int)r.dev.seg, (int)r.dev.one_trip);
}

int main() {
    char line[512];
    while (fgets(line, sizeof(line), stdin)) {
        rle::Settings s;
        size_t v[5] = {0, 0, 0, 0, 0};
        int nv = 0;
        const char* op = nullptr;
        for (char* tok = strtok(line, " \t\n"); tok; tok = strtok(nullptr, " \t\n")) {
            if (char* eq = strchr(tok, '=')) {
                const unsigned long long x = strtoull(eq + 1, nullptr, 10);
                *eq = 0;
                if (!strcmp(tok, "zerocopy")) s.zerocopy = x != 0;
                else if (!strcmp(tok, "zc_seg")) s.zc_seg = (size_t)x;
                else if (!strcmp(tok, "zc_coop")) s.zc_coop = x != 0;
                else if (!strcmp(tok, "reg_min")) s.reg_min = (size_t)x;
                else if (!strcmp(tok, "fake_devs")) s.fake_devs = (int)x;
                else return 2;
            } else if (!op) {
                op = tok;
            } else if (nv < 5) {
                v[nv++] = (size_t)strtoull(tok, nullptr, 10);
            }
        }
        if (!op) continue;
        if (!strcmp(op, "compress") && nv == 1) {
            print_call(rle::route_compress(v[0], s));
        } else if (!strcmp(op, "decompress") && nv == 3) {
            print_call(rle::route_decompress(v[0], v[1], v[2], s));
        } else if (!strcmp(op, "append") && nv == 5) {
            const rle::AppendRoute r = rle::route_append(v[0], v[1], v[2], v[3], v[4], s);
            printf("append=%s\n", r == rle::AppendRoute::Mapped ? "mapped" : r == rle::AppendRoute::SmallSplice ? "small_splice" : "large_splice");
        } else if (!strcmp(op, "readn") && nv == 2) {
            const rle::NFileRoute r = rle::route_n_file(v[0], v[1], s);
            printf("readn=%s\n", r == rle::NFileRoute::Mapped ? "mapped" : r == rle::NFileRoute::StagedSeg ? "staged_seg" : "staged");
        } else {
            return 2;
        }
    }
    return 0;
}
