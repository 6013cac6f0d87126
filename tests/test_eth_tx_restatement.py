"""The restatement the transaction tests compare against (tests/_eth_tx.py) on the CPU: its independent pin is EIP-155's worked example, every number of which is a literal
here; the committed fixture (tests/golden/eth_tx_kats.json) says what the restatement says today, covers every kind and every rule, and its signed items recover to their
signers."""
import numpy as np

from tests import _ecdsa as E
from tests import _eth_tx as T
from tests import _keccak as K

SK = bytes([0x46]) * 32
FIELDS = [9, 20 * 10**9, 21000, bytes([0x35]) * 20, 10**18, b""]
RAW = bytes.fromhex("f86c098504a817c800825208943535353535353535353535353535353535353535880de0b6b3a76400008025a028ef61340bd939bc2195fe537567866003e1a15d3c71ff63e1590620aa636276"
                    "a067cbe9d8997f761aecb703304b3800ccf555c9f3dc64214b297fb1966a3b6d83")
HASH = "daf5a779ae972f972197303d7b574746c7ef83eadac0f2791ad23db92e4c8e53"
R = 0x28EF61340BD939BC2195FE537567866003E1A15D3C71FF63E1590620AA636276
S_ = 0x67CBE9D8997F761AECB703304B3800CCF555C9F3DC64214B297FB1966A3B6D83


def test_eip155_worked_example():
    assert T.signing_data(0, FIELDS, 1).hex() == "ec098504a817c800825208943535353535353535353535353535353535353535880de0b6b3a764000080018080"
    raw, h, r, s, parity = T.build(0, SK, 1, fields=FIELDS)
    assert len(RAW) == 110 and raw == RAW and h.hex() == HASH and (r, s, parity) == (R, S_, 0)
    assert T.parse(RAW) == (bytes.fromhex(HASH), R, S_, 0, 1, 0)
    assert K.keccak256(RAW).hex() == "33469b22e9f636356c4160a87eb19df52b7412e8eac32a4a55ffe88ea8350788"
    q = E.recover(bytes.fromhex(HASH), R, S_, 0, E.LOW_S)
    assert q == E.mul(int.from_bytes(SK, "big"))
    eip55 = K.eip55(K.address_of(q))
    assert (eip55.decode() if isinstance(eip55, bytes) else eip55) == "0x9d8A62f656a8d1615C1294fd71e9CFb3E4855A4F"
    e = T.load_kats()["eip155"]
    assert (e["raw"], e["hash"], e["v"], e["sender"]) == (RAW.hex(), HASH, 37, "0x9d8A62f656a8d1615C1294fd71e9CFb3E4855A4F")


def test_rlp_forms():
    assert T.rlp(0) == b"\x80" and T.rlp(0x7F) == b"\x7f" and T.rlp(0x80) == b"\x81\x80" and T.rlp(b"") == b"\x80" and T.rlp([]) == b"\xc0"
    assert T.rlp(b"dog") == b"\x83dog" and T.rlp([b"cat", b"dog"]) == b"\xc8\x83cat\x83dog" and T.rlp(1024) == b"\x82\x04\x00"
    assert T.rlp(bytes(55))[:1] == b"\xb7" and T.rlp(bytes(56))[:2] == b"\xb8\x38" and T.rlp([bytes(55)])[:2] == b"\xf8\x38" and T.rlp(bytes(256))[:3] == b"\xb9\x01\x00"
    for enc, want in ((b"\x05", (False, 0, 1)), (b"\x80", (False, 1, 1)), (b"\x81\x80", (False, 1, 2)), (b"\x81\x7f", None), (b"\xb8\x37" + bytes(55), None),
                      (b"\xb8\x38" + bytes(56), (False, 2, 58)), (b"\xb9\x00\x38" + bytes(56), None), (b"\xc1", None), (b"\xc1\x80", (True, 1, 2)), (b"", None),
                      (b"\xf8", None), (b"\xf8\x38" + bytes(55), None)):
        assert T.read_header(enc, 0, len(enc)) == want, enc.hex()


def test_the_fixture_is_what_the_restatement_says():
    kats = T.load_kats()["items"]
    assert 257 <= len(kats) <= 400
    kinds, invalid = set(), 0
    for e in kats:
        raw = bytes.fromhex(e["raw"])
        p = T.parse(raw)
        if e["status"] == T.INVALID:
            invalid += 1
            assert p is None and int(e["r"], 16) == 0 and int(e["hash"], 16) == 0, e["name"]
            continue
        assert p == (bytes.fromhex(e["hash"]), int(e["r"], 16), int(e["s"], 16), e["v"], int(e["chain_id"]), e["tx_type"]), e["name"]
        kinds.add((p[5], p[4] != 0))
        if e["sk"]:
            assert E.recover(p[0], p[1], p[2], p[3], 0) == E.mul(int(e["sk"], 16)), e["name"]
            assert (E.recover(p[0], p[1], p[2], p[3], E.LOW_S) is None) == e["high_s"], e["name"]
    assert kinds >= {(0, False), (0, True), (1, True), (2, True), (3, True), (4, True)} and invalid >= 80
    assert any(e["high_s"] for e in kats) and any(e["status"] == T.OK and int(e["r"], 16) == 0 for e in kats)
    assert {int(e["chain_id"]) for e in kats} >= {0, 1, 127, 128, 255, 256, 2**32, 2**63 - 18, 2**64 - 1}
    assert max(len(e["raw"]) for e in kats) // 2 > 65536


def test_batch_form_and_rejected_offsets():
    kats = T.load_kats()["items"]
    raws = [bytes.fromhex(e["raw"]) for e in kats if len(e["raw"]) < 2000][:40]
    txs, off = T.pack(raws)
    out = T.parse_batch(txs, off)
    for i, raw in enumerate(raws):
        p = T.parse(raw)
        assert out["status"][i] == (T.OK if p else T.INVALID)
        if p:
            assert out["hash"][i].tobytes() == p[0] and int(out["chain_id"][i]) == p[4]
    bad = off.copy()
    bad[3] = bad[5]                                                          # item 3 runs backwards
    cut = T.parse_batch(txs, bad, txs_bytes=int(off[20]))
    assert cut["status"][3] == T.INVALID and not cut["hash"][3].any() and (cut["status"][20:] == T.INVALID).all() and np.array_equal(cut["status"][6:20], out["status"][6:20])
