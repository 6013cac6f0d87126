"""The façades of the seed derivation in Python (zk-nullifier-sig_amd/plume.py: pbkdf2_sha512, mnemonic_to_seed, mnemonic_to_address; capi.Engine.bip39_seed_batch,
bip39_accounts) and in C++ (include/plume.hpp, tests/abi_cpp/kdf_test.cpp): the Hardhat / Anvil sentence and BIP-39's TREZOR vector give their published seeds; the
sentence ALONE gives the three default accounts, keys and addresses; the device form's keys sign on the device and the signatures recover the same addresses; a str is
NFKD-normalised as BIP-39 says; and an item refused for its offsets comes out of bip39_accounts all zero with status 128 among derived neighbours."""
import hashlib
import json
import subprocess
import unicodedata
from pathlib import Path

import numpy as np
import pytest

from tests import _kdf as D

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
HD = json.loads((ROOT / "tests" / "golden" / "hd_kats.json").read_text())["known"]["hardhat"]
EIP55 = (b"0xf39Fd6e51aad88F6F4ce6aB8827279cffFb92266", b"0x70997970C51812dc3A010C7d01b50e0d17dc79C8", b"0x3C44CdDdB6a900fa2b585dd299e03d12FA4293BC")
PATHS = [f"{HD['account_path']}/{i}" for i in range(3)]


@pytest.fixture(scope="module")
def eng():
    import zk_nullifier_sig_amd as plume
    e = plume.Engine(0)
    yield e
    e.close()


def test_python_facade(eng):
    import zk_nullifier_sig_amd as plume
    assert HD["mnemonic"] == D.HARDHAT_MNEMONIC and HD["account_path"] == "m/44'/60'/0'/0"
    assert plume.mnemonic_to_seed(D.HARDHAT_MNEMONIC, engine=eng).hex() == HD["seed"]
    assert plume.mnemonic_to_seed(D.HARDHAT_MNEMONIC.encode(), b"", eng).hex() == HD["seed"]
    assert plume.mnemonic_to_seed(D.TREZOR_MNEMONIC, "TREZOR", eng).hex() == D.TREZOR_SEED
    for c, want in D.RFC_STYLE.items():
        assert plume.pbkdf2_sha512("password", b"salt", c, engine=eng).hex() == want
        assert plume.pbkdf2_sha512(b"password", "salt", c, 20, eng).hex() == want[:40]
    # the seed feeds hd_master as it is
    ms, mc = plume.hd_master(plume.mnemonic_to_seed(D.HARDHAT_MNEMONIC, engine=eng), eng)
    assert tuple(b.hex() for b in plume.hd_derive(ms, mc, HD["account_path"], eng)) == (HD["account_sk"], HD["account_chain"])
    for i, kid in enumerate(HD["children"]):
        assert plume.mnemonic_to_address(D.HARDHAT_MNEMONIC, PATHS[i], engine=eng).hex() == kid["address"]
    assert plume.mnemonic_to_address(D.HARDHAT_MNEMONIC, engine=eng).hex() == HD["children"][0]["address"]
    assert plume.mnemonic_to_address(D.HARDHAT_MNEMONIC, passphrase="x", engine=eng).hex() != HD["children"][0]["address"]
    # a str is NFKD-normalised and UTF-8 encoded: a composed character hashes as its decomposition; bytes are taken as given
    sentence, phrase = "café naïve Å", "über ﬁ"
    nfkd = lambda s: unicodedata.normalize("NFKD", s).encode()  # noqa: E731
    assert nfkd(phrase) != phrase.encode() and nfkd(sentence) != sentence.encode()
    want = hashlib.pbkdf2_hmac("sha512", nfkd(sentence), b"mnemonic" + nfkd(phrase), 2048)
    assert plume.mnemonic_to_seed(sentence, phrase, eng) == want == plume.mnemonic_to_seed(nfkd(sentence), nfkd(phrase), eng)
    assert plume.mnemonic_to_seed(sentence.encode(), phrase.encode(), eng) == hashlib.pbkdf2_hmac("sha512", sentence.encode(), b"mnemonic" + phrase.encode(), 2048) != want
    assert plume.pbkdf2_sha512(phrase, sentence, 3, engine=eng) == hashlib.pbkdf2_hmac("sha512", nfkd(phrase), nfkd(sentence), 3)
    with pytest.raises(plume.PlumeHipError):
        plume.pbkdf2_sha512(b"p", b"s", 0, engine=eng)
    with pytest.raises(ValueError):
        plume.mnemonic_to_address(D.HARDHAT_MNEMONIC, "m/", engine=eng)


def test_accounts_from_the_sentence_alone(eng):
    res = eng.bip39_accounts([D.HARDHAT_MNEMONIC], path=PATHS, addr_format="eip55")
    assert not res["status"].any() and set(res) == {"sk", "status", "chain", "pk", "address"}
    for i, kid in enumerate(HD["children"]):
        assert res["sk"][i].tobytes().hex() == kid["sk"] and res["address"][i].tobytes() == EIP55[i] and EIP55[i][2:].lower().decode() == kid["address"]
    # n sentences with one path; index rows instead of strings
    many = eng.bip39_accounts([D.HARDHAT_MNEMONIC, D.TREZOR_MNEMONIC, D.HARDHAT_MNEMONIC.encode()], path=[0x8000002C, 0x8000003C, 0x80000000, 0, 1], want=("address",))
    assert not many["status"].any() and set(many) == {"sk", "status", "address"}
    assert many["sk"][0].tobytes().hex() == many["sk"][2].tobytes().hex() == HD["children"][1]["sk"] and many["address"][0].tobytes().hex() == HD["children"][1]["address"]
    assert many["sk"][1].tobytes() != many["sk"][0].tobytes() and many["sk"][1].any()
    # a passphrase makes another wallet
    other = eng.bip39_accounts([D.HARDHAT_MNEMONIC], "TREZOR", PATHS[0], want=("address",))
    assert other["status"][0] == 0 and other["address"][0].tobytes().hex() != HD["children"][0]["address"]


def test_device_accounts_sign_on_the_device_and_recover_their_addresses(eng):
    import torch
    res = eng.bip39_accounts([D.HARDHAT_MNEMONIC], path=PATHS, device=True, want=("address",))
    n, dev = 3, res["sk"].device
    assert all(isinstance(v, torch.Tensor) and v.device == dev for v in res.values()) and int(res["status"].count_nonzero()) == 0
    digest = torch.from_numpy(np.random.default_rng(39).integers(0, 256, (n, 32), dtype=np.uint8)).to(dev)
    z = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
    r, s, v, st, pk, addr, rst = z(n, 32), z(n, 32), z(n), z(n), z(n, 64), z(n, 20), z(n)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    eng.ecdsa_sign_batch_device(n, digest, res["sk"], None, r, s, v, st, stream=stream)            # the derived sk tensor, no host copy
    eng.ecdsa_recover_batch_device(n, digest, r, s, v, None, pk, addr, rst, low_s=True, stream=stream)
    stream.synchronize()
    assert int(st.count_nonzero()) == 0
    got = addr.cpu().numpy()
    for i, kid in enumerate(HD["children"]):
        assert got[i].tobytes().hex() == kid["address"] == res["address"][i].cpu().numpy().tobytes().hex()


def test_a_refused_item_comes_out_of_the_chain_all_zero(eng):
    words = [D.HARDHAT_MNEMONIC.encode(), D.TREZOR_MNEMONIC.encode(), D.HARDHAT_MNEMONIC.encode(), b"four", D.HARDHAT_MNEMONIC.encode()]
    buf = np.frombuffer(b"".join(words), np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.uint64)
    off[2] = off[1] - 3                                     # item 1 runs backwards; item 2 starts three bytes early and is another sentence for it
    off[4] = len(buf) + 1                                   # item 3 reaches past the buffer; item 4 runs backwards from there
    res = eng.bip39_accounts((buf, off), path=PATHS[0])
    assert list(res["status"]) == [0, D.BAD_INPUT, 0, D.BAD_INPUT, D.BAD_INPUT]
    for k in ("sk", "chain", "pk", "address"):
        assert not res[k][[1, 3, 4]].any() and res[k][0].any() and res[k][2].any(), k
    assert res["sk"][0].tobytes().hex() == HD["children"][0]["sk"] and res["address"][0].tobytes().hex() == HD["children"][0]["address"]
    # what a zero seed WOULD derive is a real-looking key: the mask is what keeps it in
    sk0, chain0, st0 = eng.hd_master_batch(np.zeros((1, 64), np.uint8))
    assert st0[0] == 0 and sk0.any()
    dev = eng.bip39_accounts((buf, off), path=PATHS[0], device=True, want=())
    assert dev["status"].cpu().numpy().tolist() == [0, D.BAD_INPUT, 0, D.BAD_INPUT, D.BAD_INPUT] and not dev["sk"].cpu().numpy()[[1, 3, 4]].any()


def test_cpp_facade(tmp_path):
    import zk_nullifier_sig_amd as plume
    hx = lambda b: b.hex() if b else "-"  # noqa: E731
    rows = [("seed", hx(D.HARDHAT_MNEMONIC.encode()), "-", HD["seed"]), ("seed", hx(D.TREZOR_MNEMONIC.encode()), hx(b"TREZOR"), D.TREZOR_SEED)]
    long_sentence = (D.TREZOR_MNEMONIC + " " + D.HARDHAT_MNEMONIC).encode()          # longer than a block: the key is hashed first
    rows.append(("seed", hx(long_sentence), hx(b"p" * 200), hashlib.pbkdf2_hmac("sha512", long_sentence, b"mnemonic" + b"p" * 200, 2048).hex()))
    for c, want in D.RFC_STYLE.items():
        rows.append(("pbkdf2", hx(b"password"), hx(b"salt"), str(c), "64", want))
    rows.append(("pbkdf2", "-", "-", "3", "33", hashlib.pbkdf2_hmac("sha512", b"", b"", 3, 33).hex()))
    rows.append(("pbkdf2", hx(bytes(range(129))), hx(bytes(256)), "2", "1", hashlib.pbkdf2_hmac("sha512", bytes(range(129)), bytes(256), 2, 1).hex()))
    vectors = tmp_path / "vectors.txt"
    vectors.write_text("".join(" ".join(r) + "\n" for r in rows))
    exe = tmp_path / "kdf_test"
    libdir = plume.library_path().parent
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests" / "abi_cpp" / "kdf_test.cpp"), "-L", str(libdir),
                    "-lplume_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe), str(vectors)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "kdf_test ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
