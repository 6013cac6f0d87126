#!/usr/bin/env python3
"""Writes tests/golden/kdf_kats.json: the known answers the PBKDF2 tests pin (python tests/golden/make_kdf_kats.py).  Every value is computed with hashlib here and
ASSERTED equal to the published one while the file is written: BIP-39's first vector ("abandon" x 11 "about", passphrase TREZOR), the Hardhat / Anvil sentence (its seed
is tests/golden/hd_kats.json's), and PBKDF2-HMAC-SHA512("password", "salt") at one and two iterations."""
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from tests import _kdf as D  # noqa: E402


def main():
    hd = json.loads((ROOT / "tests" / "golden" / "hd_kats.json").read_text())["known"]["hardhat"]
    assert hd["mnemonic"] == D.HARDHAT_MNEMONIC
    kats = []

    def add(name, password, salt, iterations, bip39, want):
        got = hashlib.pbkdf2_hmac("sha512", password, (b"mnemonic" if bip39 else b"") + salt, iterations, 64).hex()
        assert got == want, (name, got)
        kats.append({"name": name, "password": password.decode(), "salt": salt.decode(), "bip39": bip39, "iterations": iterations, "out": got})

    add("bip39_trezor_vector_1", D.TREZOR_MNEMONIC.encode(), b"TREZOR", 2048, True, D.TREZOR_SEED)
    add("hardhat", D.HARDHAT_MNEMONIC.encode(), b"", 2048, True, hd["seed"])
    for c, want in D.RFC_STYLE.items():
        add(f"password_salt_{c}", b"password", b"salt", c, False, want)
    (ROOT / "tests" / "golden" / "kdf_kats.json").write_text(json.dumps({"kats": kats}, indent=1) + "\n")


if __name__ == "__main__":
    main()
