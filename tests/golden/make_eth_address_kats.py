#!/usr/bin/env python3
"""Writes tests/golden/eth_address_kats.json: the public Keccak-256 and Ethereum-address vectors the address tests pin (python tests/golden/make_eth_address_kats.py).
The digests and addresses below are typed in from public sources (the Keccak team's test vectors, the well-known addresses of the secret keys 1, 2, 3, EIP-55's own
examples); the public keys are computed by the oracle.  The script refuses to write a file that the restatement in tests/_keccak.py does not reproduce."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from oracle import plume_oracle as O  # noqa: E402
from tests import _keccak as K  # noqa: E402

KECCAK256 = [("", "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"),
             ("abc", "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45")]
ADDRESSES = [(1, "0x7E5F4552091A69125d5DfCb7b8C2659029395Bdf"), (2, "0x2B5AD5c4795c026514f8317c7a215E218DcCD6cF"), (3, "0x6813Eb9362372EEF6200f3b1dbC3f819671cBA69")]
EIP55 = ["0x5aAeb6053F3E94C9b9A09f33669435E7Ef1BeAed", "0xfB6916095ca1df60bB79Ce92cE3Ea74c37c5d359", "0x52908400098527886E0F7030069857D2E4169EE7",
         "0xde709f2102306220921060314715629080e2fb77"]

out = {"keccak256": [{"msg_utf8": m, "digest": d} for m, d in KECCAK256], "addresses": [], "eip55": EIP55}
for m, d in KECCAK256:
    assert K.keccak256(m.encode()).hex() == d, m
for sk, addr in ADDRESSES:
    pk = O.pt_bytes(O.pt_mul(sk, (O.GX, O.GY)))
    assert K.eip55(K.address_of(K.decode_pk(pk))) == addr, sk
    out["addresses"].append({"sk": sk, "pk": pk.hex(), "pk_sec1": O.sec1_compress(O.pt_from_bytes(pk)).hex(), "address": addr})
for a in EIP55:
    assert K.eip55(bytes.fromhex(a[2:])) == a, a
(ROOT / "tests" / "golden" / "eth_address_kats.json").write_text(json.dumps(out, indent=1) + "\n")
print("wrote eth_address_kats.json")
