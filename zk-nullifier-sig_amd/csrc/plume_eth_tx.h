// The senders of raw Ethereum transactions (plume_eth_tx_parse_batch / plume_eth_tx_sender_batch, include/plume_hip.h): item i = txs[tx_off[i] .. tx_off[i + 1]) is one
// signed transaction as it travels on the wire; the lane frames it, hashes the UNSIGNED payload the sender signed and hands (hash, r, s, v) to the recover stages.
// THIS IS A SENDER RECOVERY, NOT A CONSENSUS DECODER: only the envelope, the top-level framing and the signature fields are checked.  The contents of every other field --
// the nested access, blob-hash and authorization lists included -- are skipped by their header and copied verbatim into the hash.  A transaction a node accepts gets the same
// sender here; one a node rejects for an inner field may still get one.
//
// RLP: first byte 00-7f a one-byte string, the byte itself; 80-b7 a string of b - 0x80 bytes; b8-bf L = b - 0xb7 big-endian length bytes, then the string; c0-f7 a list
// whose payload is b - 0xc0 bytes; f8-ff a list with L = b - 0xf7 length bytes.  A header is canonical when a one-byte string below 0x80 uses the single-byte form, the long
// form is used only for lengths above 55 and the length bytes have no leading zero.  A canonical integer is a string with no leading zero byte; zero is the empty string.
// Envelope: first byte >= 0xc0 is a legacy transaction (tx_type 0): one list that covers the item, 9 items (nonce, gasPrice, gasLimit, to, value, data, v, r, s).  First byte
// 01, 02, 03, 04 (EIP-2930, EIP-1559, EIP-4844 in its canonical form, EIP-7702; tx_type is that byte): the rest is one list that covers it, 11, 12, 14, 13 items, the first
// chainId, the last three yParity, r, s.  Anything else -- the empty item, 00, 05-7f, 80-bf -- is invalid; so is the EIP-4844 network wrapper, by its item count.
// Framing: the outer header and every top-level header canonical, every item inside the payload, the items tile it exactly with the exact count; v / yParity, r, s and a typed
// chainId canonical integers, r and s at most 32 bytes, legacy v and typed chainId at most 8, yParity 0 or 1.
// Legacy v: 27 / 28 -> parity v - 27, chain_id 0 (unprotected); v >= 37 -> parity (v - 35) & 1, chain_id (v - 35) >> 1 (1 .. 2^63 - 18); every other value is invalid.
// Signing hash, with body = the input slice from the first top-level item to the start of v / yParity and list(x) = the canonical list header of len(x), then x:
//     legacy, unprotected   Keccak-256(list(body))
//     legacy, EIP-155       Keccak-256(list(body || rlp_int(chain_id) || 80 80))
//     typed                 Keccak-256(type || list(body))
// i.e. a prefix of at most 10 bytes, a slice of the input, a suffix of at most 11 bytes and the pad: keccak_stream (plume_keccak.h), absorbed the way k_eth_message_hash
// absorbs its own -- literal state indices, aligned 8-byte loads with a funnel shift inside the slice, edges from selects, no byte-indexed array, the block loop a vote.
// 1 <= r, s < n, the low-s rule and "no point with x = r" are NOT checked here: they belong to the recover stages (plume_ecdsa.h).
// An invalid item -- one whose offsets msg_span rejects included, and such an item never reads txs -- writes zero in every record and status PLUME_ETH_TX_INVALID.
// Every value is public: plain branches.  Compiles as plain C++ for the host (tests/eth_tx, tests/hostsim), like the other headers.
#pragma once
#include "plume_keccak.h"

#define PLUME_ETHTXK_OK 1u             // PLUME_ETH_TX_* (include/plume_hip.h)
#define PLUME_ETHTXK_INVALID 3u

namespace plume {

struct EthTxArgs {
    uint32_t n;
    const uint8_t* txs; const uint64_t* tx_off;       // n + 1 offsets
    uint64_t txs_bytes;
    uint8_t *hash, *r, *s;            // 32 bytes per item, at any byte offset
    uint8_t* v;                       // 1 byte per item: the parity
    uint64_t* chain_id;               // or NULL
    uint8_t *tx_type, *status;        // 1 byte per item, or NULL
};

// one RLP header at p, with `avail` bytes from p to the end of what encloses it
struct rlp_item {
    bool list;
    uint32_t hlen, plen;              // header and payload bytes (a one-byte string below 0x80 is its own payload: hlen 0)
};
PLUME_HD bool rlp_header(rlp_item& it, const uint8_t* p, uint32_t avail) {
    it.list = false; it.hlen = 0; it.plen = 0;
    if (avail == 0) return false;
    const uint32_t b = p[0];
    if (b < 0x80u) { it.plen = 1; return true; }
    it.list = b >= 0xc0u;
    const uint32_t t = b - (it.list ? 0xc0u : 0x80u);                                    // 0 .. 63
    if (t <= 55u) {
        it.hlen = 1; it.plen = t;
        if (t > avail - 1u) return false;
        return it.list || t != 1u || p[1] >= 0x80u;                                      // a one-byte string below 0x80 has the single-byte form
    }
    const uint32_t L = t - 55u;                                                          // 1 .. 8 length bytes
    if (L > 4u || L > avail - 1u) return false;                                          // (no leading zero: five bytes are 2^32 at least, more than any item holds)
    uint32_t len = 0;
    PLUME_UNROLL for (uint32_t k = 0; k < 4; k++) len = k < L ? (len << 8) | p[1 + k] : len;
    it.hlen = 1u + L; it.plen = len;
    if (p[1] == 0u || len <= 55u) return false;
    return len <= avail - it.hlen;
}
// a canonical integer of at most 8 bytes: a string whose payload has no leading zero
PLUME_HD bool rlp_uint64(uint64_t& v, const rlp_item& it, const uint8_t* payload) {
    v = 0;
    if (it.list || it.plen > 8u) return false;
    if (it.plen && payload[0] == 0u) return false;
    PLUME_UNROLL for (uint32_t k = 0; k < 8; k++) v = k < it.plen ? (v << 8) | payload[k] : v;
    return true;
}
// a canonical integer of at most 32 bytes as the eight memory-order words of its 32 big-endian bytes, left-padded
PLUME_HD bool rlp_uint256(uint32_t w[8], const rlp_item& it, const uint8_t* payload) {
    PLUME_UNROLL for (int k = 0; k < 8; k++) w[k] = 0u;
    if (it.list || it.plen > 32u) return false;
    if (it.plen && payload[0] == 0u) return false;
    const uint32_t pad = 32u - it.plen;
    PLUME_UNROLL for (uint32_t k = 0; k < 32; k++) {
        const uint32_t b = k >= pad ? (uint32_t)payload[k - pad] : 0u;
        w[k >> 2] |= b << (8 * (k & 3));
    }
    return true;
}
// byte b as byte k of the 16 little-endian bytes (lo, hi)
PLUME_HD void lane_put(uint64_t& lo, uint64_t& hi, uint32_t k, uint32_t b) {
    if (k < 8) lo |= (uint64_t)b << (8 * k); else hi |= (uint64_t)b << (8 * (k - 8));
}
// the number of bytes of v's shortest big-endian form (0 for 0)
PLUME_HD uint32_t be_bytes(uint64_t v) {
    uint32_t nb = 0;
    PLUME_UNROLL for (int k = 0; k < 8; k++) nb += (v >> (8 * k)) != 0 ? 1u : 0u;
    return nb;
}
// appends the canonical list header of a payload of L bytes at byte k of (lo, hi); returns the bytes written (1 .. 9)
PLUME_HD uint32_t rlp_put_list_header(uint64_t& lo, uint64_t& hi, uint32_t k, uint64_t L) {
    if (L <= 55u) { lane_put(lo, hi, k, 0xc0u + (uint32_t)L); return 1; }
    const uint32_t nb = be_bytes(L);
    lane_put(lo, hi, k, 0xf7u + nb);
    PLUME_NOUNROLL for (uint32_t j = 0; j < nb; j++) lane_put(lo, hi, k + 1 + j, (uint32_t)(L >> (8 * (nb - 1 - j))) & 0xFFu);
    return 1 + nb;
}
// appends rlp_int(v), v != 0, at byte k of (lo, hi); returns the bytes written (1 .. 9)
PLUME_HD uint32_t rlp_put_uint(uint64_t& lo, uint64_t& hi, uint32_t k, uint64_t v) {
    if (v < 0x80u) { lane_put(lo, hi, k, (uint32_t)v); return 1; }
    const uint32_t nb = be_bytes(v);
    lane_put(lo, hi, k, 0x80u + nb);
    PLUME_NOUNROLL for (uint32_t j = 0; j < nb; j++) lane_put(lo, hi, k + 1 + j, (uint32_t)(v >> (8 * (nb - 1 - j))) & 0xFFu);
    return 1 + nb;
}

// what the framing of one item gives
struct eth_tx_fields {
    uint32_t r[8], s[8];              // memory-order words of the 32 big-endian bytes
    uint32_t parity, type;
    uint64_t chain_id;
};
// frames tx[0 .. len): false = invalid (f and st are then unspecified); st is the stream of the signing hash over tx, closed
PLUME_HD bool eth_tx_frame(eth_tx_fields& f, keccak_stream& st, const uint8_t* tx, uint32_t len) {
    if (len == 0) return false;
    const uint32_t b0 = tx[0];
    const bool legacy = b0 >= 0xc0u;
    if (!legacy && (b0 < 1u || b0 > 4u)) return false;
    f.type = legacy ? 0u : b0;
    const uint32_t nitems = legacy ? 9u : b0 == 1u ? 11u : b0 == 2u ? 12u : b0 == 3u ? 14u : 13u;
    const uint32_t lst = legacy ? 0u : 1u;                                               // where the list starts
    rlp_item outer;
    if (!rlp_header(outer, tx + lst, len - lst) || !outer.list || outer.hlen + outer.plen != len - lst) return false;
    const uint32_t first = lst + outer.hlen;                                             // the first top-level item; the payload ends with the item
    uint32_t cur = first, vpos = 0;
    uint64_t chain = 0, vval = 0;
    PLUME_NOUNROLL for (uint32_t k = 0; k < nitems; k++) {
        rlp_item it;
        if (!rlp_header(it, tx + cur, len - cur)) return false;
        const uint8_t* payload = tx + cur + it.hlen;
        if (k == 0 && !legacy) { if (!rlp_uint64(chain, it, payload)) return false; }
        else if (k + 3 == nitems) { vpos = cur; if (!rlp_uint64(vval, it, payload)) return false; }
        else if (k + 2 == nitems) { if (!rlp_uint256(f.r, it, payload)) return false; }
        else if (k + 1 == nitems) { if (!rlp_uint256(f.s, it, payload)) return false; }
        cur += it.hlen + it.plen;
    }
    if (cur != len) return false;
    bool eip155 = false;
    if (legacy) {
        if (vval == 27u || vval == 28u) { f.parity = (uint32_t)vval - 27u; chain = 0; }
        else if (vval >= 37u) { f.parity = (uint32_t)(vval - 35u) & 1u; chain = (vval - 35u) >> 1; eip155 = true; }
        else return false;
    } else {
        if (vval > 1u) return false;
        f.parity = (uint32_t)vval;
    }
    f.chain_id = chain;
    keccak_stream_init(st, tx + first, vpos - first);
    if (eip155) {
        st.S = rlp_put_uint(st.s0, st.s1, 0, chain);
        lane_put(st.s0, st.s1, st.S, 0x80u); lane_put(st.s0, st.s1, st.S + 1, 0x80u);
        st.S += 2;
    }
    if (!legacy) { st.p0 = b0; st.P = 1; }
    st.P += rlp_put_list_header(st.p0, st.p1, st.P, (uint64_t)st.len + st.S);
    keccak_stream_close(st);
    return true;
}

// lane i of k_eth_tx_parse
PLUME_HD void eth_tx_parse_item(const EthTxArgs& a, uint32_t i) {
    uint64_t o0; uint32_t len;
    const bool span = msg_span(o0, len, a.tx_off, i, a.txs_bytes);                       // rejected offsets: invalid, txs never read
    eth_tx_fields f = {};
    keccak_stream st;
    const bool ok = span && eth_tx_frame(f, st, a.txs + o0, len);
    if (!ok) { keccak_stream_init(st, a.txs, 0); st.total = st.last = 0; st.nblk = 0; }
    uint32_t rec[16];
    PLUME_UNROLL for (int k = 8; k < 16; k++) rec[k] = 0u;
    PLUME_UNROLL for (int k = 0; k < 8; k++) rec[k] = ok ? f.r[k] : 0u;                    // the signature fields first: they need not live across the permutations
    recover_store<32>(a.r + 32 * (size_t)i, rec);
    PLUME_UNROLL for (int k = 0; k < 8; k++) rec[k] = ok ? f.s[k] : 0u;
    recover_store<32>(a.s + 32 * (size_t)i, rec);
    a.v[i] = (uint8_t)(ok ? f.parity : 0u);
    if (a.chain_id) a.chain_id[i] = ok ? f.chain_id : 0ull;
    if (a.tx_type) a.tx_type[i] = (uint8_t)(ok ? f.type : 0u);
    if (a.status) a.status[i] = (uint8_t)(ok ? PLUME_ETHTXK_OK : PLUME_ETHTXK_INVALID);
    keccak_stream_digest(rec, st, a.txs, a.txs + a.txs_bytes);                           // every lane: the block loop is a vote (an invalid lane absorbs nothing: all zero)
    recover_store<32>(a.hash + 32 * (size_t)i, rec);
}

}  // namespace plume
