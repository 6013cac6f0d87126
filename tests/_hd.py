"""A restatement of plume_hd_master_batch, plume_hd_derive_priv_batch and plume_hd_derive_pub_batch (include/plume_hip.h) in plain Python, shared by the key-derivation
tests: BIP-32 on secp256k1 from hmac / hashlib and the point arithmetic of tests/_ecdsa (held against the oracle's in tests/test_hd_restatement.py); the batch functions
mirror the ABI, statuses and zeroing included.  Nothing here is taken from the library's code.  Its independent pins are BIP-32's test vector 1 -- values and base58 strings,
whose checksums guard the digits -- and the default accounts of the Hardhat / Anvil mnemonic (tests/test_hd_restatement.py); tests/golden/hd_kats.json holds what it says
of seeded batches."""
import hashlib
import hmac
import json
from pathlib import Path

import numpy as np

from tests import _ecdsa as E
from tests import _ecdsa_sign as S
from tests import _keccak as K

N = E.N
OK, BAD_SCALAR, NO_KEY, HARDENED_PUB = 0, 2, 32, 64                           # PLUME_STATUS_*
MAX_DEPTH, SHARED_PARENT, SHARED_PATH = 8, 1, 2                              # PLUME_HD_*
H = 2**31
KATS = Path(__file__).resolve().parent / "golden" / "hd_kats.json"
b32 = E.b32

# BIP-32 test vector 1
V1_SEED = bytes(range(16))
V1 = {"m": ("e8f32e723decf4051aefac8e2c93c9c5b214313817cdb01a1494b917c8436b35", "873dff81c02f525623fd1fe5167eac3a55a049de3d314bb42ee227ffed37d508",
            "xprv9s21ZrQH143K3QTDL4LXw2F7HEK3wJUD2nW2nRk4stbPy6cq3jPPqjiChkVvvNKmPGJxWUtg6LnF5kejMRNNU3TGtRBeJgk33yuGBxrMPHi"),
      "m/0'": ("edb2e14f9ee77d26dd93b4ecede8d16ed408ce149b6cd80b0715a2d911a0afea", "47fdacbd0f1097043b78c63c20c34ef4ed9a111d980047ad16282c7ae6236141",
               "xprv9uHRZZhk6KAJC1avXpDAp4MDc3sQKNxDiPvvkX8Br5ngLNv1TxvUxt4cV1rGL5hj6KCesnDYUhd7oWgT11eZG7XnxHrnYeSvkzY7d2bhkJ7"),
      "m/0'/1": ("3c6cb8d0f6a264c91ea8b5030fadaa8e538b020f0a387421a12de9319dc93368", "2a7857631386ba23dacac34180dd1983734e444fdbf774041578e9b6adb37c19",
                 "xprv9wTYmMFdV23N2TdNG573QoEsfRrWKQgWeibmLntzniatZvR9BmLnvSxqu53Kw1UmYPxLgboyZQaXwTCg8MSY3H2EU4pWcQDnRnrVA1xe8fs")}
# the Hardhat / Anvil default accounts
HARDHAT_MNEMONIC = b"test test test test test test test test test test test junk"
HARDHAT_SEED = "9dfc3c64c2f8bede1533b6a79f8570e5943e0b8fd1cf77107adf7b72cef42185d564a3aee24cab43f80e3c4538087d70fc824eabbad596a23c97b6ee8322ccc0"
HARDHAT_ACCOUNT_PATH = "m/44'/60'/0'/0"
HARDHAT_ACCOUNT = ("dd23ca549a97cb330b011aebb674730df8b14acaee42d211ab45692699ab8ba5", "236a4a5d77e29cc09182a8a6c9d288cb04e638fcd0743bbc068c16665d1e4d2c")
HARDHAT_CHILDREN = (("ac0974bec39a17e36ba4a6b4d238ff944bacb478cbed5efcae784d7bf4f2ff80", "f39fd6e51aad88f6f4ce6ab8827279cfffb92266"),
                    ("59c6995e998f97a5a0044966f0945389dc9e86dae88c7a8412f4603b6b78690d", "70997970c51812dc3a010c7d01b50e0d17dc79c8"),
                    ("5de4111afa1a4b94908f83103eb1f1706367c2e68ca870fc3fb9a804cdab365a", "3c44cdddb6a900fa2b585dd299e03d12fa4293bc"))
INDEX_EDGES = (0, 1, 2**31 - 1, 2**31, 2**31 + 44, 2**32 - 1)


def hardhat_seed() -> bytes:
    return hashlib.pbkdf2_hmac("sha512", HARDHAT_MNEMONIC, b"mnemonic", 2048)


def g_mul(k: int):
    """k G as an affine pair, None for k = 0 mod n: the window table of tests/_ecdsa_sign (32 additions)"""
    acc = None
    for w, row in enumerate(S._g_windows()):
        d = ((k % N) >> (8 * w)) & 0xFF
        if d:
            acc = E._add(acc, row[d])
    return E._affine(acc)


def ser_p(pt) -> bytes:
    return bytes([2 + (pt[1] & 1)]) + b32(pt[0])


def _I(chain: bytes, data: bytes):
    d = hmac.new(chain, data, hashlib.sha512).digest()
    return int.from_bytes(d[:32], "big"), d[32:]


def master(seed: bytes):
    """(k, chain) or None"""
    il, ir = _I(b"Bitcoin seed", seed)
    return None if il == 0 or il >= N else (il, ir)


def priv_tweak(il: int, k_par: int):
    """the child scalar, or None: IL >= n or the sum is zero"""
    if il >= N:
        return None
    k = (il + k_par) % N
    return k or None


def pub_tweak(il: int, K_par):
    """the child point, or None: IL >= n or the sum is the identity"""
    if il >= N:
        return None
    return E._affine(E._add(_jac(g_mul(il)), _jac(K_par)))


def _jac(pt):
    return None if pt is None else (pt[0], pt[1], 1)


def ckd_priv(k: int, chain: bytes, i: int):
    """(k_i, c_i) or None"""
    data = (b"\x00" + b32(k) if i >= H else ser_p(g_mul(k))) + i.to_bytes(4, "big")
    il, ir = _I(chain, data)
    kc = priv_tweak(il, k)
    return None if kc is None else (kc, ir)


def ckd_pub(K_pt, chain: bytes, i: int):
    """(K_i, c_i), None (no key) -- the caller rejects hardened indices"""
    il, ir = _I(chain, ser_p(K_pt) + i.to_bytes(4, "big"))
    Kc = pub_tweak(il, K_pt)
    return None if Kc is None else (Kc, ir)


def parse_path(path: str):
    """the indices of "m/44'/60'/0'/0/3" or "0/3"; ' and h both mean hardened"""
    parts = path.split("/")
    if parts and parts[0] == "m":
        parts = parts[1:]
    out = []
    for p in parts:
        hard = p.endswith("'") or p.endswith("h")
        num = p[:-1] if hard else p
        if not num.isdigit() or int(num) >= H:
            raise ValueError(f"bad path component {p!r}")
        out.append(int(num) + (H if hard else 0))
    if not 0 < len(out) <= MAX_DEPTH:
        raise ValueError("depth must be 1 .. 8")
    return out


def derive(k: int, chain: bytes, path):
    for i in (parse_path(path) if isinstance(path, str) else path):
        node = ckd_priv(k, chain, i)
        if node is None:
            return None
        k, chain = node
    return k, chain


_B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"


def base58check_decode(s: str) -> bytes:
    v = 0
    for ch in s:
        v = v * 58 + _B58.index(ch)
    raw = v.to_bytes((v.bit_length() + 7) // 8, "big")
    raw = b"\x00" * (len(s) - len(s.lstrip("1"))) + raw
    body, check = raw[:-4], raw[-4:]
    if hashlib.sha256(hashlib.sha256(body).digest()).digest()[:4] != check:
        raise ValueError("base58 checksum")
    return body


def parse_xkey(s: str):
    """(private?, depth, child_number, chain, key bytes) of an xprv / xpub string"""
    b = base58check_decode(s)
    if len(b) != 78 or b[:4] not in (bytes.fromhex("0488ade4"), bytes.fromhex("0488b21e")):
        raise ValueError("not an xprv / xpub")
    private = b[:4] == bytes.fromhex("0488ade4")
    if private and b[45] != 0:
        raise ValueError("xprv key byte")
    return private, b[4], int.from_bytes(b[9:13], "big"), b[13:45], (b[46:78] if private else b[45:78])


# ------------------------------------------------------------------------------------------------------------- the batch forms
def _rows(a, width):
    a = np.frombuffer(a, np.uint8) if isinstance(a, (bytes, bytearray)) else np.ascontiguousarray(a, dtype=np.uint8)
    return a.reshape(-1, width)


def master_batch(seed, seed_len):
    """(sk uint8[n, 32], chain uint8[n, 32], status uint8[n])"""
    seed = _rows(seed, seed_len)
    n = len(seed)
    sk, chain, status = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    for i in range(n):
        node = master(seed[i].tobytes())
        if node is None:
            status[i] = NO_KEY
        else:
            sk[i] = np.frombuffer(b32(node[0]), np.uint8)
            chain[i] = np.frombuffer(node[1], np.uint8)
    return sk, chain, status


def _outputs(n, pk_format, addr_format):
    return (np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8), np.zeros((n, K.PK_WIDTH[pk_format]), np.uint8),
            np.zeros((n, K.ADDR_WIDTH[addr_format]), np.uint8), np.zeros(n, np.uint8))


def _fill(i, pt, chain, pk, address, chain_out, pk_format, addr_format):
    chain_out[i] = np.frombuffer(chain, np.uint8)
    pk[i] = np.frombuffer(E.pk_record(pt, pk_format), np.uint8)
    address[i] = np.frombuffer(K.record_of(K.address_of(pt), addr_format), np.uint8)


def derive_priv_batch(parent_sk, parent_chain, path, depth, flags=0, pk_format="affine64", addr_format="raw20", n=None):
    """(child_sk, child_chain, child_pk, address, status) as include/plume_hip.h defines them; n: the item count when both arrays are shared"""
    parent_sk, parent_chain = _rows(parent_sk, 32), _rows(parent_chain, 32)
    path = np.ascontiguousarray(path, dtype=np.uint32).reshape(-1, depth)
    n = n if n is not None else len(path) if not flags & SHARED_PATH else len(parent_sk)
    sk, chain, pk, address, status = _outputs(n, pk_format, addr_format)
    for i in range(n):
        row = 0 if flags & SHARED_PARENT else i
        k, c = int.from_bytes(parent_sk[row].tobytes(), "big"), parent_chain[row].tobytes()
        if not 1 <= k < N:
            status[i] = BAD_SCALAR
            continue
        node = derive(k, c, [int(x) for x in path[0 if flags & SHARED_PATH else i]])
        if node is None:
            status[i] = NO_KEY
            continue
        sk[i] = np.frombuffer(b32(node[0]), np.uint8)
        _fill(i, g_mul(node[0]), node[1], pk, address, chain, pk_format, addr_format)
    return sk, chain, pk, address, status


def derive_pub_batch(parent_pk, parent_chain, path, depth, flags=0, pk_format="affine64", addr_format="raw20", n=None):
    """(child_pk, child_chain, address, status)"""
    parent_pk, parent_chain = _rows(parent_pk, K.PK_WIDTH[pk_format]), _rows(parent_chain, 32)
    path = np.ascontiguousarray(path, dtype=np.uint32).reshape(-1, depth)
    n = n if n is not None else len(path) if not flags & SHARED_PATH else len(parent_pk)
    _, chain, pk, address, status = _outputs(n, pk_format, addr_format)
    for i in range(n):
        row = 0 if flags & SHARED_PARENT else i
        pt, c = K.decode_pk(parent_pk[row].tobytes(), pk_format), parent_chain[row].tobytes()
        if pt is None:
            status[i] = BAD_SCALAR
            continue
        for idx in (int(x) for x in path[0 if flags & SHARED_PATH else i]):
            if idx >= H:
                status[i] = HARDENED_PUB
                break
            node = ckd_pub(pt, c, idx)
            if node is None:
                status[i] = NO_KEY
                break
            pt, c = node
        if status[i] == 0:
            _fill(i, pt, c, pk, address, chain, pk_format, addr_format)
    return pk, chain, address, status


def seeded_nodes(n, seed):
    """n valid (sk, chain) pairs as uint8[n, 32] arrays"""
    rng = np.random.default_rng(seed)
    sk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    sk[:, 0] &= 0x7F                                                 # below n, and never zero in practice
    return sk, rng.integers(0, 256, (n, 32), dtype=np.uint8)


def seeded_paths(n, depth, seed):
    """uint32[n, depth]: the index edges and random indices, hardened and not, mixed along both axes"""
    rng = np.random.default_rng(seed)
    path = rng.integers(0, 2**32, (n, depth), dtype=np.uint64).astype(np.uint32)
    edge = rng.integers(0, 2 * len(INDEX_EDGES), (n, depth))
    for j, e in enumerate(INDEX_EDGES):
        path[edge == j] = e
    return path


def pk_of(sk_rows, pk_format="affine64"):
    return np.stack([np.frombuffer(E.pk_record(g_mul(int.from_bytes(r.tobytes(), "big")), pk_format), np.uint8) for r in _rows(sk_rows, 32)])


def load_kats():
    return json.loads(KATS.read_text())
