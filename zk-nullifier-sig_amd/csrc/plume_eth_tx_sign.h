// The producer of raw Ethereum transactions (plume_eth_tx_sign_batch, include/plume_hip.h): item i = txs[tx_off[i] .. tx_off[i + 1]) is the UNSIGNED serialization a
// wallet passes around -- exactly the bytes whose Keccak-256 the sender signs -- and what comes out is the signed transaction as it travels on the wire, the form
// plume_eth_tx.h parses.  THIS IS A SIGNER OF WELL-FRAMED PAYLOADS, NOT A CONSENSUS ENCODER: the envelope, the outer header and every top-level header are checked by the
// parser's rules (rlp_header); inner fields are skipped by their header and copied verbatim.
// Unsigned forms: first byte >= 0xc0 is legacy, one list that covers the item, with 6 items (nonce, gasPrice, gasLimit, to, value, data: unprotected) or 9 (EIP-155: the
// seventh chainId, a canonical integer in 1 .. 2^63 - 18, the eighth and ninth each exactly the empty string 80; nine items with anything else there are invalid, so a signed
// transaction given as input is).  First byte 01, 02, 03, 04: the rest is one list that covers it, 8, 9, 11, 10 items (the signed count less three), the first chainId, a
// canonical integer of at most 8 bytes.  Anything else is invalid.
// Two lane bodies, one item per lane, with the untouched stages of plume_ecdsa_sign.h between them:
//   eth_tx_sign_frame     frames the item; chain_id and a packed word (first top-level item, end of body, type, EIP-155, valid) go to staging the context owns; the staged
//                         hash is Keccak-256 of the whole item -- keccak_stream with no prefix and no suffix, the block loop a vote; an invalid lane absorbs nothing and
//                         stages the zero hash (what the signer makes of it is discarded below)
//   eth_tx_sign_assemble  with body = the input from the first top-level item to the end of the last unsigned field (EIP-155: to the start of chainId), v' = 27 + parity,
//                         35 + 2 chainId + parity or the parity itself, tail = rlp_int(v') || rlp_int(r) || rlp_int(s) (at most 9 + 33 + 33 bytes):
//                             legacy   list(body || tail)            typed   type || list(body || tail)
//                         into slot i = out + (tx_off[i] - tx_off[0]) + 68 i, len_i + 68 bytes long; out_len[i] is the signed length, the rest of the slot is zero.
//                         status: 0, the signer's bits, or PLUME_ST_BAD_TX alone (framing, rejected offsets, a slot that reaches past out_bytes -- the last two write no
//                         byte of out), or PLUME_ST_IDENTITY for the one v that 64 bits do not hold (chainId 2^63 - 18 with parity 1: v = 2^64).  Any status: an
//                         all-zero slot, out_len 0, zero in every optional record.
// Why 68: the payload gains at most 1 + 33 + 33 bytes (an EIP-155 item trades rlp_int(chainId) 80 80 for rlp_int(v'), at most two bytes longer than rlp_int(chainId): never
// a net gain), and a growth of at most 67 crosses at most one of the header thresholds 55/56, 255/256, 65535/65536: one more byte.
// Everything goes through ONE writer (slot_sink): bytes arrive as little-endian 64-bit groups and leave as aligned 8-byte stores, byte stores only at the two ragged ends of
// the slot -- neighbours own the rest of those words.  The body comes in by keccak_load_lane (two aligned loads and a funnel shift) where the words lie inside txs, by byte
// loads at the edges.  r and s are shifted as four named lanes; nothing is a byte-indexed array.  The lane puts exactly len_i + 68 bytes, so it cannot leave its slot.
// Every value the assemble branches on is public: the framing and a released signature.  Compiles as plain C++ for the host (tests/eth_tx_sign, tests/hostsim).
#pragma once
#include "plume_eth_tx.h"

#define PLUME_ST_BAD_TX 16u            // PLUME_STATUS_BAD_TX (include/plume_hip.h)
#define PLUME_ETHTXK_SIGN_GROWTH 68u   // PLUME_ETH_TX_SIGN_GROWTH
#define PLUME_ETHTXK_SIGN_STAGE 114u   // staging bytes per item: chain_id 8 | frame 8 | hash 32 | r 32 | s 32 | v 1 | status 1, arrays in that order

namespace plume {

struct EthTxSignArgs {
    uint32_t n;
    const uint8_t* txs; const uint64_t* tx_off;       // n + 1 offsets
    uint64_t txs_bytes;
    // staging (context-owned, aligned arrays)
    uint64_t *st_chain, *st_frame;    // per item: chain id; first | body_end << 8 | type << 40 | eip155 << 48 | valid << 49
    uint8_t* st_hash;                 // 32 B / item: what the sign stages sign
    const uint8_t *st_r, *st_s, *st_v, *st_status;    // what they wrote (assemble only)
    // the caller's arrays (assemble only), at any byte offset
    uint8_t* out; uint64_t out_bytes;
    uint32_t* out_len;
    uint8_t *hash, *r, *s, *v;        // or NULL
    uint64_t* chain_id;               // or NULL
    uint8_t* tx_type;                 // or NULL
    uint8_t* status;
};

struct eth_tx_unsigned {
    uint32_t first, body_end, type;
    bool eip155;
    uint64_t chain_id;
};
// frames the unsigned item tx[0 .. len): false = invalid (f is then unspecified)
PLUME_HD bool eth_tx_frame_unsigned(eth_tx_unsigned& f, const uint8_t* tx, uint32_t len) {
    if (len == 0) return false;
    const uint32_t b0 = tx[0];
    const bool legacy = b0 >= 0xc0u;
    if (!legacy && (b0 < 1u || b0 > 4u)) return false;
    f.type = legacy ? 0u : b0;
    const uint32_t maxitems = legacy ? 9u : b0 == 1u ? 8u : b0 == 2u ? 9u : b0 == 3u ? 11u : 10u;
    const uint32_t lst = legacy ? 0u : 1u;
    rlp_item outer;
    if (!rlp_header(outer, tx + lst, len - lst) || !outer.list || outer.hlen + outer.plen != len - lst) return false;
    f.first = lst + outer.hlen;
    uint32_t cur = f.first, k = 0, cpos = len;
    uint64_t chain = 0;
    PLUME_NOUNROLL for (; k < maxitems && cur < len; k++) {
        rlp_item it;
        if (!rlp_header(it, tx + cur, len - cur)) return false;
        const uint8_t* payload = tx + cur + it.hlen;
        if (legacy ? k == 6u : k == 0u) { cpos = cur; if (!rlp_uint64(chain, it, payload)) return false; }
        else if (legacy && k > 6u) { if (it.list || it.hlen != 1u || it.plen != 0u) return false; }      // exactly 80
        cur += it.hlen + it.plen;
    }
    if (cur != len) return false;
    f.eip155 = legacy && k == 9u;
    if (legacy ? (k != 6u && k != 9u) : k != maxitems) return false;
    if (f.eip155 && (chain < 1u || chain > 0x7FFFFFFFFFFFFFEEull)) return false;                       // 1 .. 2^63 - 18: v fits 64 bits
    f.chain_id = f.eip155 || !legacy ? chain : 0ull;
    f.body_end = f.eip155 ? cpos : len;
    return true;
}

// lane i of k_eth_tx_sign_frame
PLUME_HD void eth_tx_sign_frame_item(const EthTxSignArgs& a, uint32_t i) {
    uint64_t o0; uint32_t len;
    const bool span = msg_span(o0, len, a.tx_off, i, a.txs_bytes);                       // rejected offsets: invalid, txs never read
    eth_tx_unsigned f = {};
    const bool ok = span && eth_tx_frame_unsigned(f, a.txs + o0, len);
    keccak_stream st;
    keccak_stream_init(st, a.txs + o0, ok ? len : 0u);
    keccak_stream_close(st);
    if (!ok) { st.total = st.last = 0; st.nblk = 0; }
    a.st_chain[i] = ok ? f.chain_id : 0ull;
    a.st_frame[i] = ok ? (uint64_t)f.first | ((uint64_t)f.body_end << 8) | ((uint64_t)f.type << 40) | ((uint64_t)(f.eip155 ? 1u : 0u) << 48) | (1ull << 49) : 0ull;
    uint32_t dg[8];
    keccak_stream_digest(dg, st, a.txs, a.txs + a.txs_bytes);                            // every lane: the block loop is a vote (an invalid lane absorbs nothing: all zero)
    PLUME_UNROLL for (int k = 0; k < 8; k++) ((uint32_t*)(a.st_hash + 32 * (size_t)i))[k] = dg[k];
}

// ------------------------------------------------------------------------------------------------ the slot writer
// Bytes of one slot in order.  w is the aligned word that holds the next byte, acc its bytes so far, fill how many of its eight are decided, lead how many of them (the
// first word of a slot that starts mid-word) belong to the neighbour in front and are never stored.
struct slot_sink {
    uint8_t* w;
    uint64_t acc;
    uint32_t fill, lead;
};
PLUME_HD void sink_open(slot_sink& k, uint8_t* dst) {
    const uint32_t o = (uint32_t)((uintptr_t)dst & 7u);
    k.w = dst - o; k.acc = 0; k.fill = o; k.lead = o;
}
PLUME_HD void sink_store_bytes(uint8_t* w, uint64_t acc, uint32_t from, uint32_t to) {
    PLUME_UNROLL for (uint32_t b = 0; b < 8; b++) if (b >= from && b < to) w[b] = (uint8_t)(acc >> (8 * b));
}
// nb <= 8 bytes, the low bytes of v (the bytes above them zero)
PLUME_HD void sink_put(slot_sink& k, uint64_t v, uint32_t nb) {
    k.acc |= v << (8 * k.fill);
    const uint32_t f = k.fill + nb;
    if (f < 8u) { k.fill = f; return; }
    if (k.lead == 0u) *(uint64_t*)k.w = k.acc; else sink_store_bytes(k.w, k.acc, k.lead, 8u);
    k.acc = k.fill ? v >> (8 * (8u - k.fill)) : 0ull;
    k.w += 8; k.fill = f - 8u; k.lead = 0u;
}
PLUME_HD void sink_zeros(slot_sink& k, uint64_t count) {
    PLUME_NOUNROLL for (; count >= 8u; count -= 8u) sink_put(k, 0ull, 8u);
    sink_put(k, 0ull, (uint32_t)count);
}
// the ragged end of the slot
PLUME_HD void sink_close(slot_sink& k) { sink_store_bytes(k.w, k.acc, k.lead, k.fill); }

// the leading zero bytes (0 .. 32) of the 32 big-endian bytes held in memory order by the little-endian lanes q0 .. q3
PLUME_HD uint32_t rlp_int256_skip(uint64_t q0, uint64_t q1, uint64_t q2, uint64_t q3) {
    uint32_t z = 0, run = 1;                                                             // leading zero bytes: 0 .. 31
    PLUME_UNROLL for (uint32_t b = 0; b < 32; b++) {
        const uint64_t q = b < 8 ? q0 : b < 16 ? q1 : b < 24 ? q2 : q3;
        run &= ((q >> (8 * (b & 7))) & 0xFFu) == 0 ? 1u : 0u;
        z += run;
    }
    return z;
}
PLUME_HD void sink_put_int256(slot_sink& k, uint64_t q0, uint64_t q1, uint64_t q2, uint64_t q3, uint32_t z) {
    const uint32_t nb = 32u - z;                                                         // 1 .. 32 for a released signature (0: the empty string)
    const uint32_t wq = z >> 3, sh = 8u * (z & 7u);
    // the 32 bytes moved down by z: lane j = bytes z + 8 j ..
    uint64_t m0 = wq == 0 ? q0 : wq == 1 ? q1 : wq == 2 ? q2 : q3;
    uint64_t m1 = wq == 0 ? q1 : wq == 1 ? q2 : wq == 2 ? q3 : 0ull;
    uint64_t m2 = wq == 0 ? q2 : wq == 1 ? q3 : 0ull;
    uint64_t m3 = wq == 0 ? q3 : 0ull;
    if (sh) {
        m0 = (m0 >> sh) | (m1 << (64u - sh)); m1 = (m1 >> sh) | (m2 << (64u - sh)); m2 = (m2 >> sh) | (m3 << (64u - sh)); m3 >>= sh;
    }
    if (!(nb == 1u && (m0 & 0xFFu) < 0x80u)) sink_put(k, 0x80u + nb, 1u);
    sink_put(k, m0, nb < 8u ? nb : 8u);
    if (nb > 8u) sink_put(k, m1, nb < 16u ? nb - 8u : 8u);
    if (nb > 16u) sink_put(k, m2, nb < 24u ? nb - 16u : 8u);
    if (nb > 24u) sink_put(k, m3, nb - 24u);
}
PLUME_HD uint64_t lane_load8(const uint8_t* p) {                                         // eight bytes of an aligned staging record
    return *(const uint64_t*)p;
}
// eight input bytes at p by aligned loads where the words lie inside [lo, hi), else byte by byte
PLUME_HD uint64_t body_load8(const uint8_t* p, const uint8_t* lo, const uint8_t* hi) {
    bool ok;
    uint64_t v = keccak_load_lane(ok, p, lo, hi);
    if (!ok) { PLUME_UNROLL for (uint32_t b = 0; b < 8; b++) v |= (uint64_t)p[b] << (8 * b); }
    return v;
}

// lane i of k_eth_tx_sign_assemble
PLUME_HD void eth_tx_sign_assemble_item(const EthTxSignArgs& a, uint32_t i) {
    uint64_t o0; uint32_t len;
    const bool span = msg_span(o0, len, a.tx_off, i, a.txs_bytes);
    const uint64_t base = a.tx_off[0], raw0 = a.tx_off[i];
    // the slot: only an item with sound offsets has one, and only one that ends inside out is written
    const uint64_t slot0 = raw0 - base + (uint64_t)PLUME_ETHTXK_SIGN_GROWTH * i, slot_len = (uint64_t)len + PLUME_ETHTXK_SIGN_GROWTH;
    const bool slot_ok = span && raw0 >= base && slot0 <= a.out_bytes && slot_len <= a.out_bytes - slot0;
    const uint64_t fr = a.st_frame[i];
    const bool framed = slot_ok && ((fr >> 49) & 1u) != 0;
    const uint32_t own = a.st_status[i];
    const uint32_t first = (uint32_t)fr & 0xFFu, body_end = (uint32_t)(fr >> 8), type = (uint32_t)(fr >> 40) & 0xFFu;
    const bool eip155 = ((fr >> 48) & 1u) != 0;
    const uint64_t chain = a.st_chain[i];
    const uint32_t parity = a.st_v[i] & 1u;
    // the one v that 64 bits do not hold: 35 + 2 (2^63 - 18) + 1 = 2^64.  The parser could not read it back; like R.x >= n it is a recovery id with no representation
    const bool v_over = eip155 && chain == 0x7FFFFFFFFFFFFFEEull && parity == 1u;
    const uint32_t st = !framed ? PLUME_ST_BAD_TX : own ? own : v_over ? PLUME_ST_IDENTITY : 0u;
    const bool good = st == 0u;
    const uint8_t *pr = a.st_r + 32 * (size_t)i, *ps = a.st_s + 32 * (size_t)i, *ph = a.st_hash + 32 * (size_t)i;
    uint64_t r0 = 0, r1 = 0, r2 = 0, r3 = 0, s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    if (good) {
        r0 = lane_load8(pr); r1 = lane_load8(pr + 8); r2 = lane_load8(pr + 16); r3 = lane_load8(pr + 24);
        s0 = lane_load8(ps); s1 = lane_load8(ps + 8); s2 = lane_load8(ps + 16); s3 = lane_load8(ps + 24);
    }
    uint32_t signed_len = 0;
    if (slot_ok) {
        slot_sink k;
        sink_open(k, a.out + slot0);
        if (good) {
            // the tail's first piece, rlp_int(v'), and the lengths of the other two
            uint64_t vlo = 0, vhi = 0;
            const uint64_t vv = type ? (uint64_t)parity : eip155 ? 35u + 2u * chain + parity : 27u + parity;
            uint32_t vlen;
            if (vv == 0) { vlo = 0x80u; vlen = 1; } else vlen = rlp_put_uint(vlo, vhi, 0, vv);
            const uint32_t zr = rlp_int256_skip(r0, r1, r2, r3), zs = rlp_int256_skip(s0, s1, s2, s3);
            const uint32_t rlen = (zr == 31u && (r3 >> 56) < 0x80u) ? 1u : 33u - zr, slen = (zs == 31u && (s3 >> 56) < 0x80u) ? 1u : 33u - zs;
            const uint32_t blen = body_end - first;
            const uint64_t plen = (uint64_t)blen + vlen + rlen + slen;
            uint64_t hlo = 0, hhi = 0;
            uint32_t hl = 0;
            if (type) { hlo = type; hl = 1; }
            hl += rlp_put_list_header(hlo, hhi, hl, plen);                               // at most 1 + 5 bytes here: one lane
            sink_put(k, hlo, hl);
            const uint8_t* src = a.txs + o0 + first;
            const uint8_t *lo = a.txs, *hi = a.txs + a.txs_bytes;
            uint32_t done = 0;
            PLUME_NOUNROLL for (; done + 8u <= blen; done += 8u) sink_put(k, body_load8(src + done, lo, hi), 8u);
            if (done < blen) {
                uint64_t v = 0;
                PLUME_UNROLL for (uint32_t b = 0; b < 8; b++) if (done + b < blen) v |= (uint64_t)src[done + b] << (8 * b);
                sink_put(k, v, blen - done);
            }
            sink_put(k, vlo, vlen < 8u ? vlen : 8u);
            if (vlen > 8u) sink_put(k, vhi, vlen - 8u);
            sink_put_int256(k, r0, r1, r2, r3, zr);
            sink_put_int256(k, s0, s1, s2, s3, zs);
            signed_len = hl + (uint32_t)plen;
        }
        sink_zeros(k, slot_len - signed_len);
        sink_close(k);
    }
    a.out_len[i] = signed_len;
    a.status[i] = (uint8_t)st;
    if (a.v) a.v[i] = (uint8_t)(good ? parity : 0u);
    if (a.chain_id) a.chain_id[i] = good ? chain : 0ull;
    if (a.tx_type) a.tx_type[i] = (uint8_t)(good ? type : 0u);
    uint32_t rec[16];
    PLUME_UNROLL for (int j = 8; j < 16; j++) rec[j] = 0u;
    if (a.hash) { PLUME_UNROLL for (int j = 0; j < 8; j++) rec[j] = good ? ((const uint32_t*)ph)[j] : 0u; recover_store<32>(a.hash + 32 * (size_t)i, rec); }
    if (a.r) { PLUME_UNROLL for (int j = 0; j < 4; j++) { const uint64_t q = j == 0 ? r0 : j == 1 ? r1 : j == 2 ? r2 : r3; rec[2 * j] = (uint32_t)q; rec[2 * j + 1] = (uint32_t)(q >> 32); } recover_store<32>(a.r + 32 * (size_t)i, rec); }
    if (a.s) { PLUME_UNROLL for (int j = 0; j < 4; j++) { const uint64_t q = j == 0 ? s0 : j == 1 ? s1 : j == 2 ? s2 : s3; rec[2 * j] = (uint32_t)q; rec[2 * j + 1] = (uint32_t)(q >> 32); } recover_store<32>(a.s + 32 * (size_t)i, rec); }
}

}  // namespace plume
