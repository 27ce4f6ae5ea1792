// vg_inflate.cpp — a fast one-thread gunzip for FASTA.gz ingest (RFC 1951 / 1952), written for this library.
//
// zlib's inflate delivers 250-400 MB/s of text per thread; a one-member .gz of a 4 GB FASTA therefore costs 10-15 s in
// front of a pipeline that needs 2.  This decoder keeps 64 input bits in a register, decodes literal/length and distance
// codes through two-level tables (11 + <= 4 bits and 8 + <= 7 bits), copies matches eight bytes at a time, and leaves
// the CRC-32 of the members to worker threads (chunks + crc32_combine).  It is a FAST PATH WITH A VERDICT: every
// member's CRC-32 and length are checked, and on anything it does not like (a damaged or unusual stream, a mismatch) it
// returns false and the caller inflates the file with zlib as before -- a wrong byte cannot get through unnoticed.
#include "vg_common.h"
#include <zlib.h>
#include <stdint.h>
#include <stddef.h>
#include <algorithm>
#include <string.h>
#include <stdlib.h>
#include <vector>

namespace {
struct bitreader {
    const uint8_t* in; size_t n, pos = 0; uint64_t buf = 0; int cnt = 0; bool over = false;
    inline void refill() {
        if (pos + 8 <= n) {
            uint64_t w; memcpy(&w, in + pos, 8);
            buf |= w << cnt;
            pos += (size_t)((63 - cnt) >> 3);
            cnt |= 56;
        } else {
            while (cnt <= 56) {
                if (pos < n) buf |= (uint64_t)in[pos++] << cnt; else { over = true; }     // zeros past the end: the caller checks `over`
                cnt += 8;
            }
        }
    }
    inline uint32_t peek(int k) const { return (uint32_t)(buf & ((1ULL << k) - 1)); }
    inline void drop(int k) { buf >>= k; cnt -= k; }
    inline uint32_t take(int k) { const uint32_t v = peek(k); drop(k); return v; }
};

// table entry: bits 0-7 = code length to consume (whole code, sub-table entries included), bits 8-11 = kind, bits 12-15 =
// number of extra bits behind the code (lengths, distances), bits 16-31 = value (literal, base length, base distance).  kind: 0 literal, 1 end of block, 2 length (value = index 0..28), 3 distance (value = index), 4 sub-table
// (value = offset, low byte = number of sub-table bits), 5 invalid
constexpr int LL_MAIN = 11, D_MAIN = 8;
struct huff { std::vector<uint32_t> tab; int main_bits = 0; };
inline uint32_t mk(uint32_t value, uint32_t kind, uint32_t len, uint32_t extra = 0) { return (value << 16) | (extra << 12) | (kind << 8) | len; }
inline uint32_t kind_of(uint32_t e) { return (e >> 8) & 0xf; }

const uint16_t LEN_BASE[29] = { 3,4,5,6,7,8,9,10,11,13,15,17,19,23,27,31,35,43,51,59,67,83,99,115,131,163,195,227,258 };
const uint8_t  LEN_EXTRA[29] = { 0,0,0,0,0,0,0,0,1,1,1,1,2,2,2,2,3,3,3,3,4,4,4,4,5,5,5,5,0 };
const uint16_t DIST_BASE[30] = { 1,2,3,4,5,7,9,13,17,25,33,49,65,97,129,193,257,385,513,769,1025,1537,2049,3073,4097,6145,8193,12289,16385,24577 };
const uint8_t  DIST_EXTRA[30] = { 0,0,0,0,1,1,2,2,3,3,4,4,5,5,6,6,7,7,8,8,9,9,10,10,11,11,12,12,13,13 };

// canonical Huffman code from the lengths (RFC 1951 3.2.2) into a two-level table; false = over-subscribed / empty where not allowed
bool build(huff& h, const uint8_t* lens, int n_sym, int main_bits, bool is_dist) {
    int count[16] = { 0 }; for (int i = 0; i < n_sym; ++i) count[lens[i]]++;
    count[0] = 0;
    int max_len = 0; for (int l = 1; l <= 15; ++l) if (count[l]) max_len = l;
    h.main_bits = main_bits;
    h.tab.assign((size_t)1 << main_bits, mk(0, 5, 1));
    if (max_len == 0) return is_dist;                               // no distance codes at all is legal (literals only)
    // over-subscription / completeness
    int left = 1; for (int l = 1; l <= 15; ++l) { left <<= 1; left -= count[l]; if (left < 0) return false; }
    if (left > 0 && !(max_len == 1 && count[1] == 1 && is_dist)) {
        // incomplete codes are only allowed for a single distance code of length 1
        if (!(n_sym > 0 && count[1] == 1 && max_len == 1)) return false;
    }
    uint32_t next_code[16]; { uint32_t code = 0; for (int l = 1; l <= 15; ++l) { code = (code + (uint32_t)count[l - 1]) << 1; next_code[l] = code; } }
    // (count[0] was zeroed above, so next_code[1] = 0)
    // sub-tables: codes longer than main_bits, grouped by their main_bits-bit prefix (bit-reversed: the stream is LSB first)
    std::vector<int> sub_bits((size_t)1 << main_bits, 0);
    struct sym_code { uint32_t rev; int len; int sym; };
    std::vector<sym_code> codes; codes.reserve((size_t)n_sym);
    for (int s = 0; s < n_sym; ++s) {
        const int l = lens[s]; if (!l) continue;
        uint32_t c = next_code[l]++, r = 0;
        for (int b = 0; b < l; ++b) r |= ((c >> b) & 1u) << (l - 1 - b);          // reversed: first bit of the code in bit 0
        codes.push_back({ r, l, s });
        if (l > main_bits) { int& sb = sub_bits[r & ((1u << main_bits) - 1)]; sb = std::max(sb, l - main_bits); }
    }
    for (size_t p = 0; p < sub_bits.size(); ++p) if (sub_bits[p]) {
        const size_t off = h.tab.size();
        if (off > 0xffff) return false;
        h.tab.resize(off + ((size_t)1 << sub_bits[p]), mk(0, 5, 1));
        h.tab[p] = mk((uint32_t)off, 4, (uint32_t)sub_bits[p]);
    }
    for (const sym_code& c : codes) {
        uint32_t kind, value, extra = 0;
        if (is_dist) { if (c.sym > 29) { kind = 5; value = 0; } else { kind = 3; value = DIST_BASE[c.sym]; extra = DIST_EXTRA[c.sym]; } }
        else if (c.sym < 256) { kind = 0; value = (uint32_t)c.sym; }
        else if (c.sym == 256) { kind = 1; value = 0; }
        else if (c.sym <= 285) { kind = 2; value = LEN_BASE[c.sym - 257]; extra = LEN_EXTRA[c.sym - 257]; }
        else { kind = 5; value = 0; }
        const uint32_t e = mk(value, kind, (uint32_t)c.len, extra);
        if (c.len <= main_bits) {
            for (uint32_t p = c.rev; p < (1u << main_bits); p += 1u << c.len) h.tab[p] = e;
        } else {
            const uint32_t pre = c.rev & ((1u << main_bits) - 1), sb = (uint32_t)sub_bits[pre];
            const size_t off = h.tab[pre] >> 16;
            const uint32_t hi = c.rev >> main_bits; const int hl = c.len - main_bits;
            for (uint32_t p = hi; p < (1u << sb); p += 1u << hl) h.tab[off + p] = e;
        }
    }
    // two literals per look-up where both codes fit into the main index (DNA text: codes of 2-3 bits).  kind 6: value =
    // first | second << 8, length = both codes
    if (!is_dist && main_bits == LL_MAIN) {
        const std::vector<uint32_t> one(h.tab.begin(), h.tab.begin() + ((size_t)1 << main_bits));
        for (uint32_t p = 0; p < (1u << main_bits); ++p) {
            const uint32_t e = one[p];
            if (kind_of(e) != 0) continue;
            const int l1 = (int)(e & 0xff), rem = main_bits - l1;
            if (rem < 1) continue;
            const uint32_t e2 = one[p >> l1];                          // the unknown high bits read as zeros: fine if the code is short enough
            if (kind_of(e2) != 0 || (int)(e2 & 0xff) > rem) continue;
            h.tab[p] = mk((e >> 16) | ((e2 >> 16) << 8), 6, (uint32_t)(l1 + (int)(e2 & 0xff)));
        }
    }
    return true;
}
inline uint32_t lookup(const huff& h, const bitreader& br) {
    uint32_t e = h.tab[br.peek(h.main_bits)];
    if (kind_of(e) == 4) e = h.tab[(e >> 16) + ((uint32_t)(br.buf >> h.main_bits) & ((1u << (e & 0xff)) - 1u))];
    return e;
}

struct outbuf {
    char* p = nullptr; size_t n = 0, cap = 0;
    bool room(size_t more) {
        if (n + more <= cap) return true;
        size_t want = std::max(cap + cap / 2, n + more + (1u << 20));
        char* q = (char*)realloc(p, want);
        if (!q) return false;
        p = q; cap = want; return true;
    }
};

// one deflate stream; appends to out.  false = the stream is damaged or ends early
bool inflate_stream(bitreader& br, outbuf& out, size_t member_start) {
    static huff fixed_ll, fixed_d; static bool fixed_ok = [] {
        uint8_t l[288]; for (int i = 0; i < 144; ++i) l[i] = 8; for (int i = 144; i < 256; ++i) l[i] = 9; for (int i = 256; i < 280; ++i) l[i] = 7; for (int i = 280; i < 288; ++i) l[i] = 8;
        uint8_t d[30]; for (int i = 0; i < 30; ++i) d[i] = 5;
        // (the fixed distance code has 32 code points of 5 bits, two of them unused: an incomplete code by the book; it is
        // built with its 30 symbols padded to 32 for the completeness test)
        uint8_t d32[32]; for (int i = 0; i < 32; ++i) d32[i] = 5; (void)d;
        return build(fixed_ll, l, 288, LL_MAIN, false) && build(fixed_d, d32, 32, D_MAIN, true);
    }();
    if (!fixed_ok) return false;
    huff dyn_ll, dyn_d;
    for (;;) {
        br.refill();
        const uint32_t final_blk = br.take(1), type = br.take(2);
        if (type == 0) {
            br.drop(br.cnt & 7);                                       // to the byte boundary
            br.refill();
            const uint32_t len = br.take(16), nlen = br.take(16);
            if ((len ^ 0xffffu) != nlen || br.over) return false;
            // give the bytes still in the bit buffer back to the byte stream
            size_t at = br.pos - (size_t)(br.cnt >> 3);
            if (at + len > br.n) return false;
            if (!out.room(len + 16)) return false;
            memcpy(out.p + out.n, br.in + at, len); out.n += len;
            br.pos = at + len; br.buf = 0; br.cnt = 0;
        } else if (type == 1 || type == 2) {
            const huff* LL = &fixed_ll; const huff* DD = &fixed_d;
            if (type == 2) {
                br.refill();
                const int hlit = (int)br.take(5) + 257, hdist = (int)br.take(5) + 1, hclen = (int)br.take(4) + 4;
                if (hlit > 286 || hdist > 30) return false;
                static const uint8_t ORDER[19] = { 16,17,18,0,8,7,9,6,10,5,11,4,12,3,13,2,14,1,15 };
                uint8_t cl[19] = { 0 };
                for (int i = 0; i < hclen; ++i) { br.refill(); cl[ORDER[i]] = (uint8_t)br.take(3); }
                huff hc; if (!build(hc, cl, 19, 7, false)) return false;
                uint8_t lens[286 + 30 + 16]; int i = 0; memset(lens, 0, sizeof lens);
                while (i < hlit + hdist) {
                    br.refill();
                    const uint32_t e = hc.tab[br.peek(7)];
                    const uint32_t kind = kind_of(e); uint32_t sym = e >> 16;
                    if (kind == 5 || kind == 4) return false;
                    // (the code-length alphabet has 19 symbols: all "literals" of the table)
                    br.drop((int)(e & 0xff));
                    if (sym < 16) lens[i++] = (uint8_t)sym;
                    else if (sym == 16) { if (i == 0) return false; const uint8_t prev = lens[i - 1]; int r = 3 + (int)br.take(2); if (i + r > hlit + hdist) return false; while (r--) lens[i++] = prev; }
                    else if (sym == 17) { int r = 3 + (int)br.take(3); if (i + r > hlit + hdist) return false; i += r; }
                    else if (sym == 18) { int r = 11 + (int)br.take(7); if (i + r > hlit + hdist) return false; i += r; }
                    else return false;
                }
                if (br.over || lens[256] == 0) return false;
                if (!build(dyn_ll, lens, hlit, LL_MAIN, false) || !build(dyn_d, lens + hlit, hdist, D_MAIN, true)) return false;
                LL = &dyn_ll; DD = &dyn_d;
            }
            const uint32_t* const TL = LL->tab.data(); const uint32_t* const TD = DD->tab.data();
            const uint8_t* const in = br.in; const size_t n_in = br.n;
            for (;;) {
                if (!out.room(64 * 1024)) return false;
                // Fast loop: the bit buffer lives in locals; one refill per symbol group (a literal/length code, its extra
                // bits, a distance code and its extra bits need <= 48 of the >= 56 bits a refill leaves); the table entry
                // of the NEXT symbol is loaded before the match is copied, so that load and copy overlap.
                // (the end of the input ends it too: stop drops to 0 when a refill runs dry, so a cut stream is not decoded on,
                // zeros for bits, until the output chunk is full)
                size_t stop = out.cap - 600;
                bool end_of_block = false;
                uint64_t buf = br.buf; int cnt = br.cnt; size_t pos = br.pos; bool over = br.over;
                char* const base = out.p; size_t op = out.n;
#define VG_REFILL() do { if (pos + 8 <= n_in) { uint64_t w_; memcpy(&w_, in + pos, 8); buf |= w_ << cnt; pos += (size_t)((63 - cnt) >> 3); cnt |= 56; } \
                         else { while (cnt <= 56) { if (pos < n_in) buf |= (uint64_t)in[pos++] << cnt; else { over = true; stop = 0; } cnt += 8; } } } while (0)
#define VG_SUB(T, e_, mb) do { if (kind_of(e_) == 4) e_ = (T)[((e_) >> 16) + ((uint32_t)(buf >> (mb)) & ((1u << ((e_) & 0xff)) - 1u))]; } while (0)
                VG_REFILL();
                uint32_t e = TL[buf & ((1u << LL_MAIN) - 1)];
                while (op < stop) {
                    VG_SUB(TL, e, LL_MAIN);
                    uint32_t kind = kind_of(e);
                    if (kind == 0 || kind == 6) {
                        // literals, one or two per look-up; up to three look-ups out of the same refill (3 x 15 bits at most)
                        int rounds = 0;
                        do {
                            const uint32_t v = e >> 16;
                            base[op] = (char)v; base[op + 1] = (char)(v >> 8);
                            op += kind == 6 ? 2 : 1;
                            buf >>= (e & 0xff); cnt -= (int)(e & 0xff);
                            e = TL[buf & ((1u << LL_MAIN) - 1)];
                            if (++rounds == 3) break;
                            VG_SUB(TL, e, LL_MAIN);
                            kind = kind_of(e);
                        } while (kind == 0 || kind == 6);
                        if (rounds == 3) { VG_REFILL(); e = TL[buf & ((1u << LL_MAIN) - 1)]; continue; }
                        if (cnt < 48) { VG_REFILL(); }
                        // (e is the sub-resolved entry of a non-literal here)
                    }
                    if (kind == 2) {
                        buf >>= (e & 0xff); cnt -= (int)(e & 0xff);
                        const int xl = (int)((e >> 12) & 0xf);
                        const uint32_t len = (e >> 16) + (uint32_t)(buf & ((1u << xl) - 1)); buf >>= xl; cnt -= xl;
                        uint32_t de = TD[buf & ((1u << D_MAIN) - 1)];
                        VG_SUB(TD, de, D_MAIN);
                        if (kind_of(de) != 3) return false;
                        buf >>= (de & 0xff); cnt -= (int)(de & 0xff);
                        const int xd = (int)((de >> 12) & 0xf);
                        const size_t dist = (de >> 16) + (size_t)(buf & ((1u << xd) - 1)); buf >>= xd; cnt -= xd;
                        if (dist > op - member_start) return false;             // reaches in front of the member
                        VG_REFILL();
                        e = TL[buf & ((1u << LL_MAIN) - 1)];                     // the next symbol's entry: its load overlaps the copy
                        char* dst = base + op; const char* src = dst - dist;
                        op += len;
                        if (dist >= 8) {
                            uint64_t w; memcpy(&w, src, 8); memcpy(dst, &w, 8);   // (the output has slack behind it)
                            if (len > 8) { char* const end = dst + len; src += 8; dst += 8; do { memcpy(&w, src, 8); memcpy(dst, &w, 8); src += 8; dst += 8; } while (dst < end); }
                        } else if (dist == 1) {
                            memset(dst, (unsigned char)src[0], len);
                        } else {
                            for (uint32_t k2 = 0; k2 < len; ++k2) dst[k2] = src[k2];
                        }
                        continue;
                    }
                    if (kind == 1) { buf >>= (e & 0xff); cnt -= (int)(e & 0xff); end_of_block = true; break; }
                    return false;                                              // an unused code
                }
#undef VG_REFILL
#undef VG_SUB
                br.buf = buf; br.cnt = cnt; br.pos = pos; br.over = over; out.n = op;
                if (br.over) return false;
                if (end_of_block) break;
            }
        } else return false;
        if (final_blk) return !br.over;
    }
}
}  // namespace

// The whole file: gzip members one after the other.  On success *out_p / *out_n hold the text (malloc'd: the caller frees it).
bool vg_fast_gunzip(const unsigned char* in, size_t n, int n_threads, char** out_p, size_t* out_n) {
    outbuf out;
    // the last member's ISIZE is the length of its text modulo 2^32: the size of the whole for the usual one-member file.
    // It is read before anything is verified, so it only counts as far as n bytes of deflate can reach (1032:1 at most, a
    // 258-byte match out of two bits); a trailer that asks for more is damaged and nothing is reserved for it
    if (n >= 18) { uint32_t isz; memcpy(&isz, in + n - 4, 4); if ((size_t)isz <= 1032 * n && !out.room((size_t)isz + (1u << 16))) return false; }
    struct member { size_t o0, o1; uint32_t crc; };
    std::vector<member> members;
    size_t at = 0;
    bool ok = true;
    while (at < n && ok) {
        if (n - at < 18 || in[at] != 0x1f || in[at + 1] != 0x8b || in[at + 2] != 8) { ok = false; break; }
        const unsigned flg = in[at + 3];
        size_t h = at + 10;
        if (flg & 0xe0) { ok = false; break; }
        if (flg & 4) { if (h + 2 > n) { ok = false; break; } h += 2 + ((size_t)in[h] | ((size_t)in[h + 1] << 8)); }
        if (flg & 8) { while (h < n && in[h]) ++h; ++h; }
        if (flg & 16) { while (h < n && in[h]) ++h; ++h; }
        if (flg & 2) h += 2;
        if (h >= n) { ok = false; break; }
        bitreader br{ in, n }; br.pos = h;
        const size_t o0 = out.n;
        if (!inflate_stream(br, out, o0)) { ok = false; break; }
        size_t tail = br.pos - (size_t)(br.cnt >> 3);               // first byte behind the deflate stream
        if (tail + 8 > n) { ok = false; break; }
        uint32_t crc, isz; memcpy(&crc, in + tail, 4); memcpy(&isz, in + tail + 4, 4);
        if ((uint32_t)(out.n - o0) != isz) { ok = false; break; }
        members.push_back({ o0, out.n, crc });
        at = tail + 8;
        while (at < n && in[at] == 0) ++at;                          // (zero padding behind the last member is tolerated, as by gzip)
    }
    if (ok && members.empty()) ok = false;
    if (ok) {
        // CRC-32 of every member: chunks on worker threads, combined in order
        const size_t chunk = 16u << 20;
        struct piece { size_t a, b; uint32_t crc; };
        std::vector<piece> pieces;
        for (const member& m : members) { if (m.o1 == m.o0) continue; for (size_t a = m.o0; a < m.o1; a += chunk) pieces.push_back({ a, std::min(m.o1, a + chunk), 0 }); }
        vg_parallel_for((int64_t)pieces.size(), std::min(n_threads, 32), [&](int64_t i) {
            pieces[(size_t)i].crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef*)out.p + pieces[(size_t)i].a, (uInt)(pieces[(size_t)i].b - pieces[(size_t)i].a)); });
        size_t pi = 0;
        for (const member& m : members) {
            uLong c = crc32(0L, Z_NULL, 0);
            for (; pi < pieces.size() && pieces[pi].a < m.o1; ++pi) c = crc32_combine(c, pieces[pi].crc, (z_off_t)(pieces[pi].b - pieces[pi].a));
            if ((uint32_t)c != m.crc) { ok = false; break; }
        }
    }
    if (!ok) { free(out.p); return false; }
    *out_p = out.p; *out_n = out.n;
    return true;
}
