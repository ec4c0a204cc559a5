// json_tiles_check -- the byte level of the device JSON parsers
// (rustic_core_amd/csrc/rcdc_json_tiles.h and the two grammars) on a CPU:
// reads cases on stdin, prints one result line per case
// (tests/test_json_tiles_host.py, which holds the serial reference).  Links
// nothing of HIP and nothing of librcdc.so.
//
// Cases, as whitespace-separated tokens; TEXT is hex digits, "-" when empty:
//   fold ESC TEXT
//     TEXT cut at every pair of points into three pieces, each a Chunk whose
//     bytes lie under a scattered valid mask between junk; the pieces'
//     chunk_sum composed, applied to {instr 0, depth 0} and {instr 1, depth 0}
//     -> fold NSPLITS NSAME INSTR DEPTH INSTR DEPTH     (NSAME: splits that
//        give what the first one gives, which is the one printed)
//   ev G ESC INSTR DEPTH TEXT        G: ix | tr; the state at the first byte
//     the same pieces; per piece chunk_counts, then chunk_emit with the counts
//     of the pieces before it
//     -> ev NSPLITS NSAME N0 N1 N2 N3 NEV (KIND INDEX MY0 MY1 MY2 MY3)*
//   uint MAX TEXT      -> uint OK VALUE POS AFTER   (AFTER: after_value's verdict behind it)
//   id END TEXT        -> id OK POS (WORD)*8        (the cursor ends at END <= the text's length)
//   skip OPEN POS END K N REF CLPOS CLREF CLRANK TEXT
//     -> skip OK RANK POS
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../rustic_core_amd/csrc/rcdc_ixparse.h"
#include "../rustic_core_amd/csrc/rcdc_trparse.h"

using namespace rcdc;
using namespace rcdc::jt;
typedef unsigned long long ull;

namespace {

std::string word() {
    std::string w;
    if (!(std::cin >> w)) {
        fprintf(stderr, "json_tiles_check: case cut short\n");
        exit(2);
    }
    return w;
}

ull num() { return strtoull(word().c_str(), nullptr, 10); }

std::vector<uint8_t> text() {
    const std::string w = word();
    std::vector<uint8_t> t;
    if (w == "-") return t;
    for (size_t i = 0; i + 1 < w.size(); i += 2)
        t.push_back((uint8_t)((hexval(w[i]) << 4) | hexval(w[i + 1])));
    return t;
}

// text[a, b) as a chunk: its bytes in order under a mask that `seed` picks,
// bytes that would count between them; where[slot]: the byte's index in text
Chunk piece(const std::vector<uint8_t> &t, size_t a, size_t b, uint32_t seed, uint64_t pos,
            int where[16]) {
    static const uint8_t junk[4] = {'"', '\\', '{', ']'};
    Chunk c;
    c.pos = pos;
    c.valid = 0;
    size_t left = b - a;
    for (int j = 0; j < 16; j++) {
        seed = seed * 1664525u + 1013904223u;
        // take the slot when the rest must all be taken, or on the seed's word
        const bool take = left && ((size_t)(16 - j) == left || (seed >> 16) % 3u == 0);
        where[j] = -1;
        if (take) {
            where[j] = (int)(b - left);
            c.b[j] = t[b - left];
            c.valid |= 1u << j;
            left--;
        } else {
            c.b[j] = junk[(seed >> 8) & 3u];
        }
    }
    return c;
}

// whether the byte after the chunk is escaped: chunk_sum's own rule
uint32_t esc_after(const Chunk &c, uint32_t esc) {
    for (int j = 0; j < 16; j++) {
        if (!((c.valid >> j) & 1u)) continue;
        if (esc) esc = 0u;
        else if (c.b[j] == '\\') esc = 1u;
    }
    return esc;
}

template <bool ESC>
std::vector<ull> fold(const std::vector<uint8_t> &t, size_t c1, size_t c2) {
    const size_t cut[4] = {0, c1, c2, t.size()};
    TileSum f = {0, 0, 0u};
    uint32_t esc = 0;
    for (int p = 0; p < 3; p++) {
        int where[16];
        const Chunk c = piece(t, cut[p], cut[p + 1], (uint32_t)(c1 * 31 + c2 * 7 + p), 0, where);
        f = compose(f, chunk_sum<ESC>(c, esc));
        esc = esc_after(c, esc);
    }
    const TileIn s0 = apply(TileIn{0u, 0}, f), s1 = apply(TileIn{1u, 0}, f);
    return {s0.instr, (ull)(long long)s0.depth, s1.instr, (ull)(long long)s1.depth};
}

template <bool ESC, class Grammar>
std::vector<ull> events(const std::vector<uint8_t> &t, size_t c1, size_t c2, TileIn s) {
    const size_t cut[4] = {0, c1, c2, t.size()};
    const uint32_t cap[4] = {~0u, ~0u, ~0u, ~0u};
    uint32_t my[4] = {0, 0, 0, 0}, total[4] = {0, 0, 0, 0}, esc = 0;
    std::vector<ull> ev;
    for (int p = 0; p < 3; p++) {
        int where[16];
        const uint32_t seed = (uint32_t)(c1 * 13 + c2 * 5 + p);
        const Chunk c = piece(t, cut[p], cut[p + 1], seed, 1000u * p, where);
        uint32_t n[4];
        chunk_counts<ESC, Grammar>(c, esc, s, n);
        chunk_emit<ESC, Grammar>(c, esc, s, my, cap, [&](int e, uint64_t pos, const uint32_t *m) {
            ev.insert(ev.end(), {(ull)e, (ull)where[pos - c.pos], m[0], m[1], m[2], m[3]});
        });
        for (int e = 0; e < 4; e++) {
            total[e] += n[e];
            if (my[e] != total[e]) ev.push_back(~0ull);  // emit and counts disagree
        }
        s = apply(s, chunk_sum<ESC>(c, esc));
        esc = esc_after(c, esc);
    }
    std::vector<ull> out = {total[0], total[1], total[2], total[3], ev.size() / 6};
    out.insert(out.end(), ev.begin(), ev.end());
    return out;
}

// every split of t in three: the first one's result and how many give the same
template <class F>
void splits(const char *what, const std::vector<uint8_t> &t, F one) {
    std::vector<ull> first;
    ull n = 0, same = 0;
    for (size_t c1 = 0; c1 <= t.size(); c1++)
        for (size_t c2 = c1; c2 <= t.size(); c2++) {
            const std::vector<ull> r = one(c1, c2);
            if (!n++) first = r;
            same += r == first;
        }
    printf("%s %llu %llu", what, n, same);
    for (ull v : first) printf(" %lld", (long long)v);
    printf("\n");
}

}  // namespace

int main() {
    std::string kind;
    while (std::cin >> kind) {
        if (kind == "fold") {
            const bool esc = num() != 0;
            const std::vector<uint8_t> t = text();
            splits("fold", t, [&](size_t a, size_t b) {
                return esc ? fold<true>(t, a, b) : fold<false>(t, a, b);
            });
        } else if (kind == "ev") {
            const bool ix = word() == "ix", esc = num() != 0;
            TileIn s;
            s.instr = (uint32_t)num();
            s.depth = (int32_t)num();
            const std::vector<uint8_t> t = text();
            splits("ev", t, [&](size_t a, size_t b) {
                if (ix)
                    return esc ? events<true, IxGrammar>(t, a, b, s)
                               : events<false, IxGrammar>(t, a, b, s);
                return esc ? events<true, TrGrammar>(t, a, b, s) : events<false, TrGrammar>(t, a, b, s);
            });
        } else if (kind == "uint") {
            const ull max = num();
            const std::vector<uint8_t> t = text();
            Cur c = {t.data(), 0, t.size()};
            uint64_t v = 0;
            const bool ok = parse_uint(c, max, &v);
            const ull pos = c.pos;
            bool more = false;
            const bool after = ok && after_value(c, &more);
            printf("uint %d %llu %llu %d\n", (int)ok, ok ? (ull)v : 0ull, pos, (int)after);
        } else if (kind == "id") {
            const ull end = num();
            const std::vector<uint8_t> t = text();
            Cur c = {t.data(), 0, end};
            uint32_t id[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            const bool ok = parse_id(c, id);
            printf("id %d %llu", (int)ok, (ull)c.pos);
            for (uint32_t w : id) printf(" %u", ok ? w : 0u);
            printf("\n");
        } else if (kind == "skip") {
            const int open = (int)num();
            const ull pos = num(), end = num();
            const uint32_t k = (uint32_t)num(), n = (uint32_t)num(), ref = (uint32_t)num();
            std::vector<TileClose> cl(k + 1, TileClose{0, ~0u, 0u});
            cl[k].pos = num();
            cl[k].ref = (uint32_t)num();
            cl[k].rank = (uint32_t)num();
            const std::vector<uint8_t> t = text();
            Cur c = {t.data(), pos, end};
            uint32_t rank = 0;
            const bool ok = skip_array(c, open, cl.data(), k, n, ref, &rank);
            printf("skip %d %u %llu\n", (int)ok, ok ? rank : 0u, (ull)c.pos);
        } else {
            fprintf(stderr, "json_tiles_check: unknown case %s\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
