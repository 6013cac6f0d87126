"""ctypes binding of libplume_hip.so (include/plume_hip.h) — the only way this package computes anything.

There is deliberately no fallback: if the shared library is missing, or no gfx950 GPU is visible, constructing
an Engine raises PlumeHipError.  torch is used only as plumbing (device buffers / streams) by the *_device
methods; the host-pointer methods need numpy only.
"""
import ctypes as C
import os
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
_u8p = C.POINTER(C.c_uint8)
_u64p = C.POINTER(C.c_uint64)


# the library's shipped defaults (plume_capi.hip, struct plume_ctx) -- tests that turn a knob restore these
DEFAULT_CHUNK = 1 << 20
DEFAULT_HOST_PIECE = 1 << 19
DEFAULT_HOST_FIRST_PIECE = 1 << 16
DEFAULT_HOST_TAIL_PIECE = 1 << 16
DEFAULT_SUB_BATCHES = 1


class PlumeHipError(RuntimeError):
    pass


def library_path() -> Path:
    """the in-tree build; PLUME_HIP_LIB selects another build of the same library (A/B tuning runs only)"""
    alt = os.environ.get("PLUME_HIP_LIB")
    return Path(alt).resolve() if alt else _HERE / "libplume_hip.so"


# ---------------------------------------------------------------------- the prototypes of include/plume_hip.h (ctypes only: no library is loaded here)
# GROUPS: group -> (since, what).  A group's entry points may be missing from an older build selected through PLUME_HIP_LIB (A/B runs against an earlier round): _load
# prototypes them only where the symbol exists and Engine._fn refuses the call in words (NullifierSet for its group).  "later" has no version of its own.
GROUPS = {
    "later": (None, "later entry points"),
    "nullset": ((0, 7), "persistent nullifier set"),
    "rfc6979": ((0, 8), "derived-nonce signer"),
    "selfcheck": ((0, 9), "signer self-check"),
    "recover": ((0, 10), "point recovery"),
    "eth": ((0, 11), "Ethereum addresses"),
    "ecdsa": ((0, 12), "ECDSA recovery"),
    "ecdsa_sign": ((0, 13), "ECDSA signing"),
    "eth_tx": ((0, 14), "transaction parsing"),
    "merkle": ((0, 15), "Merkle trees"),
    "eth_tx_sign": ((0, 16), "transaction signing"),
    "hd": ((0, 17), "key derivation"),
}
_VOID = "void"          # a row's restype for a function that returns nothing (None in a row means: not given, ctypes' default c_int)

# PROTOTYPES: name -> (restype, argtypes, group).  group None = every supported build has it (a missing one is ctypes' AttributeError at load); argtypes None = left unset
PROTOTYPES = {}


def _rows(group, *rows):
    for name, args, *res in rows:
        PROTOTYPES[name] = (res[0] if res else None, args, group)


vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
_rows(None,
      ("plume_last_error", None, C.c_char_p), ("plume_version", None, C.c_char_p),
      ("plume_microbench", [vp, i, i], C.c_double), ("plume_microbench_last_ticks", [C.POINTER(C.c_float)], C.c_double),
      ("plume_init", [C.POINTER(C.c_void_p), i]), ("plume_init_multi", [C.POINTER(C.c_void_p), C.POINTER(C.c_int), i]),
      ("plume_num_shards", [vp]), ("plume_shard_numa_node", [vp, i]),
      ("plume_set_host_first_piece", [vp, sz]), ("plume_set_host_register_min", [vp, sz]), ("plume_set_host_tail_piece", [vp, sz]),
      ("plume_host_alloc", [sz], C.c_void_p), ("plume_host_free", [vp]), ("plume_host_register", [vp, sz]), ("plume_host_unregister", [vp]),
      ("plume_destroy", [vp]), ("plume_set_chunk", [vp, sz]), ("plume_set_sub_batches", [vp, i]), ("plume_set_in_flight", [vp, i]))
# later entry points: an older build selected through PLUME_HIP_LIB (A/B runs against an earlier round) may lack them; the in-tree library must have them all (_load checks)
_rows("later",
      ("plume_set_sign_uniform", [vp, i]), ("plume_get_sign_uniform", [vp]), ("plume_set_host_lanes", [vp, i]), ("plume_set_eq1_short", [vp, i]),
      ("plume_set_stage_timing", [vp, i]),
      # BIP-39 seeds (library 0.18): PBKDF2-HMAC-SHA512 for a batch
      ("plume_pbkdf2_sha512_batch", [vp, i, sz, vp, vp, vp, sz, C.c_uint32, sz, vp, vp]),
      ("plume_pbkdf2_sha512_batch_device", [vp, i, sz, vp, vp, sz, vp, sz, C.c_uint32, sz, vp, vp, vp]))
_rows(None,
      ("plume_get_eq1_short", [vp, C.POINTER(C.c_size_t)]), ("plume_last_msm_clock", [vp, C.POINTER(C.c_double)]), ("plume_last_msm_kernel", [vp], C.c_char_p),
      ("plume_set_host_piece", [vp, sz]), ("plume_last_redo_tasks", [vp, C.POINTER(C.c_uint64)]),
      ("plume_last_stage_times", [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), i]),
      ("plume_verify_batch", [vp, i, sz] + [vp] * 9), ("plume_verify_batch_sec1", [vp, i, sz] + [vp] * 9), ("plume_verify_non_zk_batch", [vp, i, sz] + [vp] * 9),
      ("plume_verify_non_zk_batch_device", [vp, i, sz, vp, vp, sz] + [vp] * 8), ("plume_verify_batch_sec1_device", [vp, i, sz, vp, vp, sz] + [vp] * 8),
      ("plume_sign_batch", [vp, i, sz] + [vp] * 12), ("plume_sign_batch_sec1", [vp, i, sz] + [vp] * 12),
      ("plume_sign_batch_sec1_device", [vp, i, sz, vp, vp, sz] + [vp] * 11),
      ("plume_nullifier_first_occurrence", [vp, sz, vp, vp, vp, vp, C.POINTER(C.c_uint64)]), ("plume_nullifier_first_occurrence_device", [vp, sz, vp, vp, vp, vp, vp, vp]),
      ("plume_hash_to_curve_batch", [vp, sz] + [vp] * 4),
      ("plume_verify_batch_device", [vp, i, sz, vp, vp, sz] + [vp] * 8), ("plume_sign_batch_device", [vp, i, sz, vp, vp, sz] + [vp] * 11),
      ("plume_hash_to_curve_batch_device", [vp, sz, vp, vp, sz, vp, vp, vp]),
      ("plume_h2c_intermediates_batch", [vp, sz, vp, vp, vp, i, vp, vp, vp, vp]), ("plume_h2c_intermediates_batch_device", [vp, sz, vp, vp, sz, vp, i, vp, vp, vp, vp, vp]),
      ("plume_h2c_hints_batch", [vp, sz, vp, vp, vp, i, vp]), ("plume_h2c_hints_batch_device", [vp, sz, vp, vp, sz, vp, i, vp, vp]),
      ("plume_registers_from_be", [sz, vp, vp]), ("plume_registers_from_be_device", [vp, sz, vp, vp, vp]),
      ("plume_scalars_to_sec1_der_batch", [vp, sz, vp, vp, vp]), ("plume_scalars_to_sec1_der_batch_device", [vp, sz, vp, vp, vp, vp]),
      ("plume_sec1_der_to_scalars", [sz, vp, vp, vp]), ("plume_sec1_der_to_scalars_checked", [vp, sz, vp, vp, vp]),
      ("plume_aggregate_check", [vp, i, i, sz] + [vp] * 11),
      ("plume_aggregate_check_device", [vp, i, i, sz, vp, vp, sz] + [vp] * 7 + [C.c_uint64, vp, vp, vp]))
# the persistent nullifier set (library 0.7; an older build selected through PLUME_HIP_LIB lacks it: NullifierSet raises PlumeHipError then)
_rows("nullset",
      ("plume_nullset_create", [vp, sz, C.POINTER(C.c_void_p)]), ("plume_nullset_destroy", [vp], _VOID), ("plume_nullset_reserve", [vp, sz]), ("plume_nullset_clear", [vp]),
      ("plume_nullset_size", [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]), ("plume_nullset_insert", [vp, sz, vp, vp, vp, vp, C.POINTER(C.c_uint64)]),
      ("plume_nullset_contains", [vp, sz, vp, vp]), ("plume_nullset_export", [vp, sz, vp, C.POINTER(C.c_uint64)]),
      ("plume_nullset_insert_device", [vp, sz, vp, vp, vp, vp, vp, vp]), ("plume_nullset_contains_device", [vp, sz, vp, vp, vp]))
# derived signing nonces (library 0.8; Engine.sign_batch_rfc6979* raise PlumeHipError on an older build)
_rows("rfc6979", ("plume_sign_batch_rfc6979", [vp, i, sz] + [vp] * 12), ("plume_sign_batch_rfc6979_device", [vp, i, sz, vp, vp, sz] + [vp] * 11))
# the signer's self-check (library 0.9; Engine.set_sign_selfcheck raises PlumeHipError on an older build selected through PLUME_HIP_LIB)
_rows("selfcheck", ("plume_set_sign_selfcheck", [vp, i]), ("plume_get_sign_selfcheck", [vp]))
# point recovery (library 0.10; Engine.recover_batch* raise PlumeHipError on an older build selected through PLUME_HIP_LIB)
_rows("recover", ("plume_recover_batch", [vp, i, i, sz] + [vp] * 10), ("plume_recover_batch_device", [vp, i, i, sz, vp, vp, sz] + [vp] * 9))
# Ethereum addresses (library 0.11; Engine.eth_address_batch* raise PlumeHipError on an older build selected through PLUME_HIP_LIB)
_rows("eth", ("plume_eth_address_batch", [vp, i, i, sz] + [vp] * 4), ("plume_eth_address_batch_device", [vp, i, i, sz] + [vp] * 5))
# ECDSA public-key recovery (library 0.12; Engine.ecdsa_recover_batch* raise PlumeHipError on an older build selected through PLUME_HIP_LIB)
_rows("ecdsa", ("plume_ecdsa_recover_batch", [vp, i, i, i, sz] + [vp] * 8), ("plume_ecdsa_recover_batch_device", [vp, i, i, i, sz] + [vp] * 9))
# the digest a wallet signs and deterministic ECDSA signatures (library 0.13; Engine.eth_message_hash_batch* / ecdsa_sign_batch* raise PlumeHipError on an older build)
_rows("ecdsa_sign",
      ("plume_eth_message_hash_batch", [vp, i, sz] + [vp] * 3), ("plume_eth_message_hash_batch_device", [vp, i, sz, vp, vp, sz, vp, vp]),
      ("plume_ecdsa_sign_batch", [vp, i, sz] + [vp] * 7), ("plume_ecdsa_sign_batch_device", [vp, i, sz] + [vp] * 8))
# the senders of raw transactions (library 0.14; Engine.eth_tx_parse_batch* / eth_tx_sender_batch* raise PlumeHipError on an older build)
_rows("eth_tx",
      ("plume_eth_tx_parse_batch", [vp, sz] + [vp] * 9), ("plume_eth_tx_parse_batch_device", [vp, sz, vp, vp, sz] + [vp] * 8),
      ("plume_eth_tx_sender_batch", [vp, i, i, i, sz] + [vp] * 8), ("plume_eth_tx_sender_batch_device", [vp, i, i, i, sz, vp, vp, sz] + [vp] * 7))
# Keccak Merkle allow-lists (library 0.15; Engine.merkle_* raise PlumeHipError on an older build)
_rows("merkle",
      ("plume_merkle_leaf_batch", [vp, i, i, sz] + [vp] * 4), ("plume_merkle_leaf_batch_device", [vp, i, i, sz] + [vp] * 5),
      ("plume_merkle_tree_build", [vp, i, sz] + [vp] * 3), ("plume_merkle_tree_build_device", [vp, i, sz] + [vp] * 4),
      ("plume_merkle_proof_batch", [vp, sz, vp, sz, vp, sz, vp, vp]), ("plume_merkle_proof_batch_device", [vp, sz, vp, sz, vp, sz, vp, vp, vp]),
      ("plume_merkle_verify_batch", [vp, i, i, sz, vp, vp, sz] + [vp] * 4), ("plume_merkle_verify_batch_device", [vp, i, i, sz, vp, vp, sz] + [vp] * 5),
      ("plume_merkle_max_proof_len", [sz], C.c_void_p))                            # (a size_t: ctypes hands back None for 0)
# signing raw transactions (library 0.16; Engine.eth_tx_sign_batch* raise PlumeHipError on an older build)
_rows("eth_tx_sign",
      ("plume_eth_tx_sign_batch", [vp, i, sz] + [vp] * 13), ("plume_eth_tx_sign_batch_device", [vp, i, sz, vp, vp, sz, vp, vp, vp, sz] + [vp] * 9),
      ("plume_eth_tx_sign_out_bytes", [sz, C.c_uint64], C.c_void_p))                # (a size_t)
# BIP-32 key derivation (library 0.17; Engine.hd_* raise PlumeHipError on an older build)
_rows("hd",
      ("plume_hd_master_batch", [vp, sz, vp, sz, vp, vp, vp]), ("plume_hd_master_batch_device", [vp, sz, vp, sz, vp, vp, vp, vp]),
      ("plume_hd_derive_priv_batch", [vp, i, i, i, sz, vp, vp, vp, sz] + [vp] * 5), ("plume_hd_derive_priv_batch_device", [vp, i, i, i, sz, vp, vp, vp, sz] + [vp] * 6),
      ("plume_hd_derive_pub_batch", [vp, i, i, i, sz, vp, vp, vp, sz] + [vp] * 4), ("plume_hd_derive_pub_batch_device", [vp, i, i, i, sz, vp, vp, vp, sz] + [vp] * 5))
del vp, sz, i

_lib = None


def _load():
    # The runtime's hardware-queue pool (4 per priority level by default): streams that share a queue run their kernels one after the other, which is what defeats
    # plume_set_in_flight for callers with two streams (include/plume_hip.h).  Effective only if set before the process's first HIP call; harmless after it.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    global _lib
    if _lib is not None:
        return _lib
    p = library_path()
    if not p.exists():
        raise PlumeHipError(f"{p} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                            f"(or `make -C zk-nullifier-sig_amd/csrc`). There is no CPU fallback.")
    # torch ships its own libamdhip64.so (same SONAME as /opt/rocm's).  Whichever copy is loaded first serves the
    # whole process; loading ours first leaves torch without a usable device ("No HIP GPUs are available").  So if
    # torch is installed, let it load its runtime first; the library itself has no torch dependency.
    if not os.environ.get("PLUME_NO_TORCH_PRELOAD"):     # experiments only: run on /opt/rocm's runtime instead of the one torch bundles (tests/gpu_debug/d2h_in_library.py)
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    lib = C.CDLL(str(p))
    for name, (res, args, group) in PROTOTYPES.items():
        fn = getattr(lib, name) if group is None else getattr(lib, name, None)
        if fn is None:
            continue
        if args is not None:
            fn.argtypes = args
        if res is not None:
            fn.restype = None if res is _VOID else res
    _lib = lib
    # (the 0.13 entry points are told by their symbols: plume_version() still begins "plume_hip 0.12")
    if (_version(lib) < (0, 12) or getattr(lib, "plume_ecdsa_sign_batch", None) is None) and not os.environ.get("PLUME_HIP_LIB"):
        _lib = None
        raise PlumeHipError(f"{p} is {lib.plume_version().decode()} without plume_ecdsa_sign_batch: this module needs the 0.13 entry points (rebuild: make -C zk-nullifier-sig_amd/csrc)")
    return lib


def exported_symbols():
    """every entry point include/plume_hip.h declares (used by the CPU-side ABI test)"""
    return list(PROTOTYPES)


def pack_messages(msgs):
    """list of bytes -> (packed uint8 array, uint64 offsets[n+1])"""
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    if len(msgs):
        off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    buf = np.frombuffer(b"".join(msgs) + b"\0" * 16, dtype=np.uint8).copy()
    return buf, off


def bip39_bytes(text):
    """what BIP-39 hashes of a sentence or a passphrase: a str NFKD-normalised and UTF-8 encoded; bytes are taken as given"""
    if isinstance(text, str):
        import unicodedata
        return unicodedata.normalize("NFKD", text).encode("utf-8")
    return bytes(text)


def _np(a, width, n, name):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.size != width * n:
        raise ValueError(f"{name}: expected {n} records of {width} bytes, got {a.size} bytes")
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _ragged(msgs, msg_off):
    """(n, msgs, msg_off) of a ragged input as pack_messages returns it: contiguous uint8 bytes and n + 1 uint64 offsets"""
    msg_off = np.ascontiguousarray(msg_off, dtype=np.uint64)
    return len(msg_off) - 1, np.ascontiguousarray(msgs, dtype=np.uint8), msg_off


_SIGN_OUTPUTS = ("pk", "nullifier", "c", "s", "r_point", "hashed_to_curve_r", "status")      # in the order the sign calls take them


def _sign_outputs(n, width, out=None):
    """what a sign call writes: the caller's dict `out` as it is, or fresh arrays -- six records and the status; width: bytes per point record (64, or 33 for SEC1)"""
    if out is not None:
        return out
    o = {k: np.zeros((n, 32 if k in ("c", "s") else width), dtype=np.uint8) for k in _SIGN_OUTPUTS[:6]}
    o["status"] = np.zeros(n, dtype=np.uint8)
    return o


AGG_RESULT_BYTES = 72
# plume_recover_batch (include/plume_hip.h): the status of an item and the record formats of the recovered points
RECOVER_MISMATCH, RECOVER_MATCH, RECOVER_INVALID = 0, 1, 3
RECOVER_FMT_AFFINE64, RECOVER_FMT_SEC1, RECOVER_FMT_REGISTERS = 0, 1, 2
RECOVER_OUTPUTS = ("r_point", "hashed_to_curve_r", "hashed_to_curve")
# plume_eth_address_batch (include/plume_hip.h): the status of an item, the formats of the keys and of the address records
ETH_MISMATCH, ETH_MATCH, ETH_INVALID = 0, 1, 3
ETH_PK_FORMATS = {"affine64": (0, 64), "sec1": (1, 33)}                       # name -> (PLUME_ETH_PK_*, bytes per key)
ETH_ADDR_FORMATS = {"raw20": (0, 20), "record64": (1, 64), "eip55": (2, 42)}   # name -> (PLUME_ETH_ADDR_*, bytes per record)
# plume_ecdsa_recover_batch (include/plume_hip.h): the status of an item, the flag bits; keys and addresses come in the formats above
ECDSA_MISMATCH, ECDSA_MATCH, ECDSA_INVALID = 0, 1, 3
ECDSA_LOW_S = 1
# plume_eth_message_hash_batch (include/plume_hip.h): what is hashed;  plume_ecdsa_sign_batch: the flag bit (the status of an item is the signer's: 0, 2, 4, 8)
ETH_HASH_MODES = {"keccak256": 0, "eip191": 1}
ECDSA_SIGN_V27 = 1
# plume_eth_tx_parse_batch (include/plume_hip.h): the status of an item (plume_eth_tx_sender_batch reports the recovery's: ECDSA_*)
ETH_TX_OK, ETH_TX_INVALID = 1, 3
# plume_eth_tx_sign_batch (include/plume_hip.h): the status bit it adds to the signer's (0, 2, 4, 8) and the bytes a slot has beyond its unsigned item
STATUS_BAD_TX = 16
ETH_TX_SIGN_GROWTH = 68
# plume_hd_*_batch (include/plume_hip.h): the deepest path, the flag bits, the status bits they add to PLUME_STATUS_BAD_SCALAR (2), the first hardened index
HD_MAX_DEPTH = 8
HD_SHARED_PARENT, HD_SHARED_PATH = 1, 2
STATUS_HD_NO_KEY, STATUS_HD_HARDENED = 32, 64
HD_HARDENED = 2**31
# plume_pbkdf2_sha512_batch (include/plume_hip.h): the flag bits, the longest salt, the most iterations, the status of an item whose offsets are unsound (device form)
KDF_BIP39, KDF_SHARED_SALT = 1, 2
KDF_MAX_SALT = 256
KDF_MAX_ITERATIONS = 1 << 24
STATUS_KDF_BAD_INPUT = 128
# plume_merkle_* (include/plume_hip.h): leaf formats -> (PLUME_MERKLE_LEAF_*), the sort flag, the status of an item, the proof length of a refused index
MERKLE_LEAF_FORMATS = {"hash32": 0, "address": 1, "address_uint256": 2}
MERKLE_SORT_LEAVES = 1
MERKLE_MISMATCH, MERKLE_MATCH, MERKLE_INVALID = 0, 1, 3
MERKLE_BAD_PROOF = 255


def parse_aggregate_record(rec):
    """the 72-byte result of plume_aggregate_check (include/plume_hip.h)"""
    rec = np.asarray(rec, dtype=np.uint8)
    return dict(all_ok=bool(rec[0]), identity=bool(rec[1]), n_bad=int.from_bytes(rec[4:8].tobytes(), "little"), point=rec[8:72].tobytes())


def registers_from_be(values):
    """(.., 32) uint8 big-endian values -> (.., 4) uint64 little-endian 64-bit registers (circuits/circom/utils.ts:11-17)"""
    lib = _load()
    v = np.ascontiguousarray(values, dtype=np.uint8)
    if v.shape[-1] != 32:
        raise ValueError("values must be 32-byte records")
    out = np.zeros(v.shape[:-1] + (4,), dtype=np.uint64)
    rc = lib.plume_registers_from_be(v.size // 32, _ptr(v), _ptr(out))
    if rc != 0:
        raise PlumeHipError(f"plume_registers_from_be failed ({rc}): {lib.plume_last_error().decode()}")
    return out


def sec1_der_to_scalars(der109):
    """(n, 109) SEC1-DER secret-key records (the wasm layer's `s` / `digest_private`) -> (scalars (n, 32), ok (n,)); the STRUCTURE half of SecretKey::from_sec1_der only
    (shape + scalar range, no GPU): Engine.sec1_der_to_scalars also checks the embedded public key against scalar * G, as the reference does"""
    lib = _load()
    d = np.ascontiguousarray(der109, dtype=np.uint8).reshape(-1, 109)
    sc, ok = np.zeros((len(d), 32), dtype=np.uint8), np.zeros(len(d), dtype=np.uint8)
    rc = lib.plume_sec1_der_to_scalars(len(d), _ptr(d), _ptr(sc), _ptr(ok))
    if rc != 0:
        raise PlumeHipError(f"plume_sec1_der_to_scalars failed ({rc}): {lib.plume_last_error().decode()}")
    return sc, ok


def pinned_empty(shape, dtype=np.uint8):
    """numpy array in page-locked host memory (plume_host_alloc): the copy engines read / write it directly, so the host-pointer calls
    overlap every transfer with the neighbouring pieces' kernels.  Freed when the array (and every view of it) is gone."""
    lib = _load()
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(x) for x in shape)
    nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
    p = lib.plume_host_alloc(max(nbytes, 1))
    if not p:
        raise PlumeHipError(f"plume_host_alloc({nbytes}) failed: {lib.plume_last_error().decode()}")

    class _Owner:
        def __init__(self, ptr):
            self.ptr = ptr

        def __del__(self):
            try:
                lib.plume_host_free(self.ptr)
            except Exception:
                pass

    buf = (C.c_uint8 * max(nbytes, 1)).from_address(p)
    buf._plume_owner = _Owner(p)   # the ctypes buffer is the base object of the numpy array: it keeps the owner alive
    return np.frombuffer(buf, dtype=np.uint8, count=nbytes).view(dtype).reshape(shape)


def pinned_copy(a):
    out = pinned_empty(a.shape, a.dtype)
    out[...] = a
    return out


class Engine:
    """One context (include/plume_hip.h: plume_ctx).  Engine(k) = one GPU (plume_init; one Engine per process rank / device);
    Engine([k0, k1, ..]) = a multi-device context (plume_init_multi): the host-pointer calls shard every batch over the devices."""

    def __init__(self, device_id=None):
        lib = _load()
        if device_id is None:
            device_id = int(os.environ.get("LOCAL_RANK", "0"))
        self._lib = lib
        self._ctx = C.c_void_p()
        if isinstance(device_id, (list, tuple)):
            ids = (C.c_int * len(device_id))(*[int(d) for d in device_id])
            rc = lib.plume_init_multi(C.byref(self._ctx), ids, len(device_id))
            what = f"plume_init_multi(devices {list(device_id)})"
            self.device_ids = [int(d) for d in device_id]
            self.device_id = self.device_ids[0] if self.device_ids else 0
        else:
            rc = lib.plume_init(C.byref(self._ctx), int(device_id))
            what = f"plume_init(device {device_id})"
            self.device_id = int(device_id)
            self.device_ids = [self.device_id]
        if rc != 0:
            self._ctx = None
            raise PlumeHipError(f"{what} failed ({rc}): {lib.plume_last_error().decode()}")

    def num_shards(self):
        return int(self._lib.plume_num_shards(self._ctx))

    def shard_numa_nodes(self):
        """per shard: the NUMA node its worker thread was bound to (-1 = not bound)"""
        return [int(self._lib.plume_shard_numa_node(self._ctx, d)) for d in range(self.num_shards())]

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.plume_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise PlumeHipError(f"{what} failed ({rc}): {self._lib.plume_last_error().decode()}")

    def _fn(self, name):
        """the entry point `name`, or PlumeHipError where this build lacks its group (GROUPS).  Up to 0.12 the version string counts too; the later groups are told by
        their symbols alone: plume_version() still begins "plume_hip 0.12" """
        since, what = GROUPS.get(PROTOTYPES[name][2], (None, None))
        if since is None:
            return getattr(self._lib, name)            # no group, or "later": a missing one is ctypes' AttributeError
        fn = getattr(self._lib, name, None)
        by_version = since <= (0, 12)
        if fn is None or (by_version and _version(self._lib) < since):
            how = f"needs plume_hip >= {since[0]}.{since[1]}" if by_version else f"came with library {since[0]}.{since[1]}"
            raise PlumeHipError(f"{self._lib.plume_version().decode()} has no {what}: {name} {how} (rebuild: make -C zk-nullifier-sig_amd/csrc)")
        return fn

    def _enqueue(self, name, stream, *args):
        """a device-resident call: name(ctx, *args, stream handle) on `stream` (torch.cuda.Stream, or None = the current stream of this device); does not synchronise"""
        import torch
        fn = self._fn(name)
        st = (stream or torch.cuda.current_stream(self.device_id)).cuda_stream
        self._chk(fn(self._ctx, *args, C.c_void_p(st)), name)

    def version(self):
        return self._lib.plume_version().decode()

    def set_chunk(self, n):
        self._chk(self._lib.plume_set_chunk(self._ctx, int(n)), "plume_set_chunk")

    def set_sub_batches(self, k):
        """device-resident verify / sign: number of overlapped sub-batches per call; 1 = strictly serial launch order (per-kernel stage times)"""
        self._chk(self._lib.plume_set_sub_batches(self._ctx, int(k)), "plume_set_sub_batches")

    def set_in_flight(self, k):
        """batches in flight (plume_set_in_flight): with k = 2 the device-resident calls go in turn to two lanes of the context, so that calls issued on different streams run
        side by side (2^20 verifies: about 1 % per batch; calls of fewer than 2^17 items stay on the first lane); default 1; results do not depend on it"""
        self._chk(self._lib.plume_set_in_flight(self._ctx, int(k)), "plume_set_in_flight")

    def set_sign_uniform(self, on):
        """the signer's uniform schedule (plume_set_sign_uniform): level 1 (or True) = no branch on a digit of sk or r, level 2 = and no table address derived from
        one (every row of a window's table is read); outputs unchanged"""
        self._chk(self._lib.plume_set_sign_uniform(self._ctx, int(on)), "plume_set_sign_uniform")

    def sign_uniform(self):
        """the level this context signs at (plume_get_sign_uniform): 1 by default since library 0.4"""
        rc = self._lib.plume_get_sign_uniform(self._ctx)
        if rc < 0:
            self._chk(rc, "plume_get_sign_uniform")
        return rc

    def set_sign_selfcheck(self, mode):
        """the signer's self-check (plume_set_sign_selfcheck): 1 (or True) = every sign call verifies its own records on the GPU (verify_non_zk) before anything reaches
        the caller's arrays; an item that does not verify comes out all zero with status STATUS_SELFCHECK_FAILED (8).  0 (the default) = off"""
        self._chk(self._fn("plume_set_sign_selfcheck")(self._ctx, int(mode)), "plume_set_sign_selfcheck")

    def sign_selfcheck(self):
        """the mode this context signs with (plume_get_sign_selfcheck): 0 by default"""
        rc = self._fn("plume_get_sign_selfcheck")(self._ctx)
        if rc < 0:
            self._chk(rc, "plume_get_sign_selfcheck")
        return rc

    def set_eq1_short(self, mode):
        """the verifier's first equation where R is given: 1 = short form for calls of at least eq1_short()[1] items (csrc/plume_eis.h; the default), 3 = short form whatever the
        size, 0 = long form always, 2 = test mode (every item through the scalar stage's fallback)"""
        self._chk(self._lib.plume_set_eq1_short(self._ctx, int(mode)), "plume_set_eq1_short")

    def eq1_short(self):
        """(mode, min_items) in force on this context (plume_get_eq1_short): mode as set_eq1_short takes it, min_items = the smallest call that takes the short form in mode 1"""
        m = C.c_size_t(0)
        rc = self._lib.plume_get_eq1_short(self._ctx, C.byref(m))
        if rc < 0:
            self._chk(rc, "plume_get_eq1_short")
        return rc, int(m.value)

    def last_msm_clock_ghz(self):
        """the shader clock (GHz) the multi-scalar kernel of the last verify call ran at, sampled inside the kernel (plume_last_msm_clock; stage timing must be on), or None"""
        g = C.c_double(0.0)
        rc = self._lib.plume_last_msm_clock(self._ctx, C.byref(g))
        return float(g.value) if rc == 0 else None

    def last_msm_kernel(self):
        """the multi-scalar kernel the last verify call on this context launched (plume_last_msm_kernel): 'k_verify_msm', 'k_verify_msm_s', 'k_verify_msm_pair', or None"""
        r = self._lib.plume_last_msm_kernel(self._ctx)
        return r.decode() if r else None

    def set_host_lanes(self, lanes):
        """host-pointer calls: 1 = every piece on the context itself, 2 (default) = pieces alternate between the context and a second lane"""
        self._chk(self._lib.plume_set_host_lanes(self._ctx, int(lanes)), "plume_set_host_lanes")

    def set_host_piece(self, n):
        """host-pointer calls: items per pipelined piece (upload / compute / download overlap across pieces)"""
        self._chk(self._lib.plume_set_host_piece(self._ctx, int(n)), "plume_set_host_piece")

    def set_host_first_piece(self, n):
        self._chk(self._lib.plume_set_host_first_piece(self._ctx, int(n)), "plume_set_host_first_piece")

    def set_host_tail_piece(self, n):
        self._chk(self._lib.plume_set_host_tail_piece(self._ctx, int(n)), "plume_set_host_tail_piece")

    def set_host_register_min(self, nbytes):
        """host-pointer calls: page-lock pageable caller arrays of at least nbytes for the duration of the call (0 = never)"""
        self._chk(self._lib.plume_set_host_register_min(self._ctx, int(nbytes)), "plume_set_host_register_min")

    # ------------------------------------------------------------------ host-pointer API (numpy in, numpy out)
    def verify_non_zk_batch(self, version, msgs, msg_off, pk, nullifier, s, r_point, hashed_to_curve_r, digest_private, out=None):
        """plume_arkworks' verify_non_zk (rust-arkworks/src/tests.rs:28-78), batched: 1 Ok(true), 0 Ok(false), 2 Err(HashToCurveError)"""
        n, msgs, msg_off = _ragged(msgs, msg_off)
        pk, nullifier, s = _np(pk, 64, n, "pk"), _np(nullifier, 64, n, "nullifier"), _np(s, 32, n, "s")
        r_point, hashed_to_curve_r = _np(r_point, 64, n, "r_point"), _np(hashed_to_curve_r, 64, n, "hashed_to_curve_r")
        digest_private = _np(digest_private, 32, n, "digest_private")
        ok = np.zeros(n, dtype=np.uint8) if out is None else out
        self._chk(self._lib.plume_verify_non_zk_batch(self._ctx, int(version), n, _ptr(msgs), _ptr(msg_off), _ptr(pk), _ptr(nullifier), _ptr(s), _ptr(r_point),
                                                      _ptr(hashed_to_curve_r), _ptr(digest_private), _ptr(ok)), "plume_verify_non_zk_batch")
        return ok

    def aggregate_check(self, version, msgs, msg_off, pk, nullifier, c, s, r_point, hashed_to_curve_r, seed=None, mode=0):
        """Aggregate random-linear-combination pre-filter (include/plume_hip.h plume_aggregate_check): all-or-nothing and
        probabilistic, never a replacement for verify_batch.  mode 0: PlumeSignature::verify of V1 signatures; mode 1: verify_non_zk (c = digest_private).
        seed: 32 bytes the producer of the batch cannot predict (default: os.urandom).  Returns dict(all_ok, identity, n_bad, point, hash_ok, seed)."""
        import os
        n, msgs, msg_off = _ragged(msgs, msg_off)
        pk, nullifier, c, s = _np(pk, 64, n, "pk"), _np(nullifier, 64, n, "nullifier"), _np(c, 32, n, "c"), _np(s, 32, n, "s")
        r_point, hashed_to_curve_r = _np(r_point, 64, n, "r_point"), _np(hashed_to_curve_r, 64, n, "hashed_to_curve_r")
        seed = os.urandom(32) if seed is None else bytes(seed)
        if len(seed) != 32:
            raise ValueError("seed must be 32 bytes")
        sd = np.frombuffer(seed, dtype=np.uint8).copy()
        hash_ok = np.zeros(n, dtype=np.uint8)
        rec = np.zeros(AGG_RESULT_BYTES, dtype=np.uint8)
        self._chk(self._lib.plume_aggregate_check(self._ctx, int(version), int(mode), n, _ptr(msgs), _ptr(msg_off), _ptr(pk), _ptr(nullifier), _ptr(c), _ptr(s), _ptr(r_point),
                                                  _ptr(hashed_to_curve_r), _ptr(sd), _ptr(hash_ok), _ptr(rec)), "plume_aggregate_check")
        out = parse_aggregate_record(rec)
        out["hash_ok"] = hash_ok
        out["seed"] = seed
        return out

    def verify_batch(self, version, msgs, msg_off, pk, nullifier, c, s, r_point=None, hashed_to_curve_r=None, out=None):
        n, msgs, msg_off = _ragged(msgs, msg_off)
        pk, nullifier, c, s = _np(pk, 64, n, "pk"), _np(nullifier, 64, n, "nullifier"), _np(c, 32, n, "c"), _np(s, 32, n, "s")
        if version == 1:
            if r_point is None or hashed_to_curve_r is None:
                raise ValueError("V1 verification needs r_point and hashed_to_curve_r")
            r_point, hashed_to_curve_r = _np(r_point, 64, n, "r_point"), _np(hashed_to_curve_r, 64, n, "hashed_to_curve_r")
        else:
            r_point = hashed_to_curve_r = None
        ok = np.zeros(n, dtype=np.uint8) if out is None else out
        self._chk(self._lib.plume_verify_batch(self._ctx, int(version), n, _ptr(msgs), _ptr(msg_off), _ptr(pk), _ptr(nullifier), _ptr(c), _ptr(s),
                                               _ptr(r_point), _ptr(hashed_to_curve_r), _ptr(ok)), "plume_verify_batch")
        return ok

    def recover_batch(self, version, msgs, msg_off, pk, nullifier, c, s, fmt=RECOVER_FMT_AFFINE64, want=RECOVER_OUTPUTS + ("status",)):
        """r_point = s G - c pk, hashed_to_curve_r = s H - c nullifier and H = hash_to_curve(msg, pk) of every item (plume_recover_batch): what a V2 signature leaves out.
        fmt: RECOVER_FMT_AFFINE64 (n x 64 bytes), RECOVER_FMT_SEC1 (n x 33) or RECOVER_FMT_REGISTERS (n x 2 x 4 uint64, the circuit's registers).  want: which of
        r_point, hashed_to_curve_r, hashed_to_curve, status to compute.  Returns a dict of those; status[i] is RECOVER_MATCH (c is version's hash of the points),
        RECOVER_MISMATCH (points written all the same) or RECOVER_INVALID (an input is no value of the reference's types: zero records)."""
        fn = self._fn("plume_recover_batch")
        want = tuple(want)
        if not want or any(k not in RECOVER_OUTPUTS + ("status",) for k in want):
            raise ValueError("want: a non-empty subset of r_point, hashed_to_curve_r, hashed_to_curve, status")
        n, msgs, msg_off = _ragged(msgs, msg_off)
        pk, nullifier, c, s = _np(pk, 64, n, "pk"), _np(nullifier, 64, n, "nullifier"), _np(c, 32, n, "c"), _np(s, 32, n, "s")
        shape, dt = {RECOVER_FMT_AFFINE64: ((n, 64), np.uint8), RECOVER_FMT_SEC1: ((n, 33), np.uint8), RECOVER_FMT_REGISTERS: ((n, 2, 4), np.uint64)}[int(fmt)]
        o = {k: np.zeros(shape, dtype=dt) for k in RECOVER_OUTPUTS if k in want}
        if "status" in want:
            o["status"] = np.zeros(n, dtype=np.uint8)
        self._chk(fn(self._ctx, int(version), int(fmt), n, _ptr(msgs), _ptr(msg_off), _ptr(pk), _ptr(nullifier), _ptr(c), _ptr(s), _ptr(o.get("r_point")),
                     _ptr(o.get("hashed_to_curve_r")), _ptr(o.get("hashed_to_curve")), _ptr(o.get("status"))), "plume_recover_batch")
        return o

    def eth_address_batch(self, pk, expect=None, pk_format="affine64", addr_format="raw20"):
        """The Ethereum address of every public key, Keccak-256(x || y)[12:] (plume_eth_address_batch).  pk: n x 64 bytes ("affine64") or n x 33 ("sec1"); expect:
        None or n x 20 raw bytes, the address each key is claimed to have.  Returns (address, status): address is n x 20 ("raw20"), n x 64 ("record64": 44 zero bytes
        then the address, a record Engine.nullifier_set() takes as is) or n x 42 ASCII ("eip55": "0x" + checksummed hex); status[i] is ETH_MATCH (expect is None or
        equals the address), ETH_MISMATCH, or ETH_INVALID (no non-identity curve point: a zero record)."""
        fn = self._fn("plume_eth_address_batch")
        pf, P = ETH_PK_FORMATS[pk_format]
        af, W = ETH_ADDR_FORMATS[addr_format]
        pk = np.ascontiguousarray(pk, dtype=np.uint8)
        if pk.size % P:
            raise ValueError(f"pk: expected records of {P} bytes, got {pk.size} bytes")
        n = pk.size // P
        expect = None if expect is None else _np(expect, 20, n, "expect")
        address, status = np.zeros((n, W), dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        self._chk(fn(self._ctx, pf, af, n, _ptr(pk), _ptr(expect), _ptr(address), _ptr(status)), "plume_eth_address_batch")
        return address, status

    def ecdsa_recover_batch(self, hash, r, s, v, expect=None, pk_format="affine64", addr_format="raw20", low_s=False, want=("pk", "address", "status")):
        """The public key and the Ethereum address behind every ECDSA signature (plume_ecdsa_recover_batch): Ethereum's ecrecover with a one-byte v in {0, 1, 27, 28}.
        hash, r, s: n x 32 big-endian bytes; v: n bytes; expect: None or n x 20 raw bytes, the address each signer is claimed to have; low_s: s > (n - 1) / 2 is invalid
        (EIP-2).  Returns (pk, address, status) -- None for an output not named in `want`: pk is n x 64 ("affine64") or n x 33 ("sec1"), address as
        eth_address_batch writes it for addr_format, status[i] is ECDSA_MATCH (expect is None or equals the address), ECDSA_MISMATCH (pk and address are written all the
        same), or ECDSA_INVALID (v, r or s out of range, no point with x = r, or the key comes out as the identity: zero records)."""
        fn = self._fn("plume_ecdsa_recover_batch")
        pf, P = ETH_PK_FORMATS[pk_format]
        af, W = ETH_ADDR_FORMATS[addr_format]
        v = np.ascontiguousarray(v, dtype=np.uint8).reshape(-1)
        n = v.size
        hash, r, s = _np(hash, 32, n, "hash"), _np(r, 32, n, "r"), _np(s, 32, n, "s")
        expect = None if expect is None else _np(expect, 20, n, "expect")
        pk = np.zeros((n, P), dtype=np.uint8) if "pk" in want else None
        address = np.zeros((n, W), dtype=np.uint8) if "address" in want else None
        status = np.zeros(n, dtype=np.uint8) if "status" in want else None
        self._chk(fn(self._ctx, ECDSA_LOW_S if low_s else 0, pf, af, n, _ptr(hash), _ptr(r), _ptr(s), _ptr(v), _ptr(expect), _ptr(pk), _ptr(address), _ptr(status)),
                  "plume_ecdsa_recover_batch")
        return pk, address, status

    def eth_message_hash_batch(self, msgs, msg_off, mode="eip191"):
        """The digest a wallet signs for every ragged message (plume_eth_message_hash_batch): Keccak-256(msg) for mode "keccak256", Keccak-256("\\x19Ethereum Signed
        Message:\\n" || decimal(len) || msg) for "eip191" (personal_sign).  msgs, msg_off as pack_messages returns them; a mode may also be given as its integer.
        Returns n x 32 bytes."""
        fn = self._fn("plume_eth_message_hash_batch")
        n, msgs, msg_off = _ragged(msgs, msg_off)
        out = np.zeros((n, 32), dtype=np.uint8)
        self._chk(fn(self._ctx, int(ETH_HASH_MODES.get(mode, mode)), n, _ptr(msgs), _ptr(msg_off), _ptr(out)), "plume_eth_message_hash_batch")
        return out

    def ecdsa_sign_batch(self, hash, sk, aux=None, v27=False, flags=None):
        """Deterministic ECDSA signatures with a recovery id (plume_ecdsa_sign_batch): RFC 6979 nonces over the digest itself (aux: None, or n x 32 bytes of section 3.6's
        extra input), always low s.  hash, sk: n x 32 big-endian bytes.  Returns (r, s, v, status): r, s n x 32 bytes, v the parity of R's y behind the low-s flip (0 / 1,
        or 27 / 28 with v27), status[i] 0 (signed), 2 (sk outside [1, n - 1]), 4 (a degenerate outcome) or 8 (withheld by the self-check); r, s, v are zero unless
        status is 0.  flags: the raw flag word instead of v27."""
        fn = self._fn("plume_ecdsa_sign_batch")
        sk = np.ascontiguousarray(sk, dtype=np.uint8)
        if sk.size % 32:
            raise ValueError(f"sk: expected records of 32 bytes, got {sk.size} bytes")
        n = sk.size // 32
        hash = _np(hash, 32, n, "hash")
        aux = None if aux is None else _np(aux, 32, n, "aux")
        r, s = np.zeros((n, 32), dtype=np.uint8), np.zeros((n, 32), dtype=np.uint8)
        v, status = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        fl = (ECDSA_SIGN_V27 if v27 else 0) if flags is None else int(flags)
        self._chk(fn(self._ctx, fl, n, _ptr(hash), _ptr(sk), _ptr(aux), _ptr(r), _ptr(s), _ptr(v), _ptr(status)), "plume_ecdsa_sign_batch")
        return r, s, v, status

    def eth_tx_parse_batch(self, txs, tx_off):
        """What plume_ecdsa_recover_batch takes, from raw signed transactions (plume_eth_tx_parse_batch): legacy (unprotected or EIP-155) and the typed envelopes 01 - 04.
        txs, tx_off as pack_messages returns them.  Returns a dict: hash (n x 32: what the sender signed), r, s (n x 32 big-endian), v (n: the parity, 0 or 1), chain_id
        (n uint64; 0 for an unprotected legacy item), tx_type (n) and status (n: ETH_TX_OK or ETH_TX_INVALID, every record of an invalid item being zero).  A sender
        recovery, not a consensus decoder: fields other than the envelope and the signature are not inspected.  The transaction id is
        eth_message_hash_batch(txs, tx_off, "keccak256")."""
        fn = self._fn("plume_eth_tx_parse_batch")
        n, txs, tx_off = _ragged(txs, tx_off)
        out = {"hash": np.zeros((n, 32), np.uint8), "r": np.zeros((n, 32), np.uint8), "s": np.zeros((n, 32), np.uint8), "v": np.zeros(n, np.uint8),
               "chain_id": np.zeros(n, np.uint64), "tx_type": np.zeros(n, np.uint8), "status": np.zeros(n, np.uint8)}
        self._chk(fn(self._ctx, n, _ptr(txs), _ptr(tx_off), *(_ptr(out[k]) for k in ("hash", "r", "s", "v", "chain_id", "tx_type", "status"))), "plume_eth_tx_parse_batch")
        return out

    def eth_tx_sender_batch(self, txs, tx_off, expect=None, pk_format="affine64", addr_format="raw20", low_s=True, want=("pk", "address", "status")):
        """The sender of every raw signed transaction (plume_eth_tx_sender_batch): eth_tx_parse_batch into staging the context owns, then the stages of
        ecdsa_recover_batch.  expect, the formats, low_s (on by default: the rule for everything after Homestead) and `want` are that call's.  Returns (pk, address,
        status, chain_id, tx_type): status[i] is ECDSA_MATCH, ECDSA_MISMATCH or ECDSA_INVALID (the framing or the signature: zero records); chain_id and tx_type report
        the framing and are zero only for an item invalid there."""
        fn = self._fn("plume_eth_tx_sender_batch")
        pf, P = ETH_PK_FORMATS[pk_format]
        af, W = ETH_ADDR_FORMATS[addr_format]
        n, txs, tx_off = _ragged(txs, tx_off)
        expect = None if expect is None else _np(expect, 20, n, "expect")
        pk = np.zeros((n, P), dtype=np.uint8) if "pk" in want else None
        address = np.zeros((n, W), dtype=np.uint8) if "address" in want else None
        status = np.zeros(n, dtype=np.uint8) if "status" in want else None
        chain_id, tx_type = np.zeros(n, np.uint64), np.zeros(n, np.uint8)
        self._chk(fn(self._ctx, ECDSA_LOW_S if low_s else 0, pf, af, n, _ptr(txs), _ptr(tx_off), _ptr(expect), _ptr(pk), _ptr(address), _ptr(chain_id), _ptr(tx_type),
                     _ptr(status)), "plume_eth_tx_sender_batch")
        return pk, address, status, chain_id, tx_type

    def eth_tx_sign_slots(self, txs, tx_off, sk, aux=None, want=("hash", "r", "s", "v", "chain_id", "tx_type")):
        """plume_eth_tx_sign_batch as the library writes it: a dict with out (the slots: item i's at (tx_off[i] - tx_off[0]) + 68 i, len_i + 68 bytes, zero beyond
        out_len[i]), out_len (n uint32), status (n) and the records named in `want`.  txs, tx_off as pack_messages returns them: UNSIGNED transactions."""
        fn = self._fn("plume_eth_tx_sign_batch")
        n, txs, tx_off = _ragged(txs, tx_off)
        sk = _np(sk, 32, n, "sk")
        aux = None if aux is None else _np(aux, 32, n, "aux")
        nbytes = int(tx_off[n]) - int(tx_off[0]) if n else 0
        res = {"out": np.zeros(nbytes + ETH_TX_SIGN_GROWTH * n, np.uint8), "out_len": np.zeros(n, np.uint32), "status": np.zeros(n, np.uint8)}
        rec = {"hash": (n, 32), "r": (n, 32), "s": (n, 32), "v": (n,), "tx_type": (n,)}
        for k in want:
            res[k] = np.zeros(n, np.uint64) if k == "chain_id" else np.zeros(rec[k], np.uint8)
        self._chk(fn(self._ctx, 0, n, _ptr(txs), _ptr(tx_off), _ptr(sk), _ptr(aux), _ptr(res["out"]), _ptr(res["out_len"]),
                     *(_ptr(res.get(k)) for k in ("hash", "r", "s", "v", "chain_id", "tx_type")), _ptr(res["status"])), "plume_eth_tx_sign_batch")
        return res

    def eth_tx_sign_batch(self, unsigned, sk, aux=None, records=False):
        """Signed raw transactions from unsigned payloads (plume_eth_tx_sign_batch): legacy (6 items: unprotected; 9 items ending chainId, 80, 80: EIP-155) and the typed
        envelopes 01 - 04 without their last three fields.  unsigned: a list of bytes, or (txs, tx_off) as pack_messages returns them; sk: n x 32 big-endian bytes; aux:
        None, or n x 32 bytes that hedge the RFC 6979 nonce.  Returns (raw, status): raw[i] the signed item as bytes (empty unless status[i] is 0), status[i] 0 (signed),
        2, 4, 8 as ecdsa_sign_batch reports them, or STATUS_BAD_TX (16: an ill-framed item, whatever the key is).  records=True: a third value, the dict of hash, r, s,
        v (the parity), chain_id and tx_type of every item -- what eth_tx_parse_batch would say of raw[i]."""
        txs, tx_off = unsigned if isinstance(unsigned, tuple) else pack_messages([bytes(u) for u in unsigned])
        res = self.eth_tx_sign_slots(txs, tx_off, sk, aux, want=("hash", "r", "s", "v", "chain_id", "tx_type") if records else ())
        ob = res["out"].tobytes()
        base = int(tx_off[0]) if len(tx_off) else 0
        raw = [ob[int(tx_off[i]) - base + ETH_TX_SIGN_GROWTH * i:][:int(ln)] for i, ln in enumerate(res["out_len"])]
        if records:
            return raw, res["status"], {k: res[k] for k in ("hash", "r", "s", "v", "chain_id", "tx_type")}
        return raw, res["status"]

    def hd_master_batch(self, seed, seed_len=None):
        """BIP-32 master nodes (plume_hd_master_batch).  seed: n x seed_len bytes (a 2-D array, or flat with seed_len given), 16 <= seed_len <= 64.  Returns
        (sk, chain, status): n x 32 bytes each and n status bytes -- 0, or STATUS_HD_NO_KEY (32) with both records all zero."""
        fn = self._fn("plume_hd_master_batch")
        seed = np.ascontiguousarray(seed, dtype=np.uint8)
        if seed_len is None:
            if seed.ndim != 2:
                raise ValueError("seed: give an n x seed_len array, or seed_len")
            seed_len = seed.shape[1]
        if seed_len <= 0 or seed.size % int(seed_len):
            raise ValueError("seed: not a whole number of seed_len-byte records")
        n = seed.size // int(seed_len)
        sk, chain, status = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
        self._chk(fn(self._ctx, n, _ptr(seed), int(seed_len), _ptr(sk), _ptr(chain), _ptr(status)), "plume_hd_master_batch")
        return sk, chain, status

    @staticmethod
    def _hd_shape(parent, width, chain, path, name):
        """(flags, n, depth, parent, chain, path) of a derive call: a parent of ONE record or a path of ONE row is shared by every item"""
        path = np.ascontiguousarray(path, dtype=np.uint32)
        if path.ndim == 1:
            path = path.reshape(1, -1)
        parent, chain = np.ascontiguousarray(parent, dtype=np.uint8).reshape(-1, width), np.ascontiguousarray(chain, dtype=np.uint8).reshape(-1, 32)
        if len(parent) != len(chain):
            raise ValueError(f"{name}: {len(parent)} parent keys and {len(chain)} chain codes")
        n = max(len(parent), len(path))
        flags = (HD_SHARED_PARENT if len(parent) == 1 and n > 1 else 0) | (HD_SHARED_PATH if len(path) == 1 and n > 1 else 0)
        if len(parent) not in (1, n) or len(path) not in (1, n):
            raise ValueError(f"{name}: {len(parent)} parents and {len(path)} paths")
        return flags, n, path.shape[1], parent, chain, path

    def hd_derive_priv_batch(self, parent_sk, parent_chain, path, pk_format="affine64", addr_format="raw20", want=("chain", "pk", "address"), device=False):
        """BIP-32 private derivation (plume_hd_derive_priv_batch).  parent_sk, parent_chain: n x 32 bytes, or ONE record shared by every item; path: n x depth uint32
        indices (>= 2^31: hardened), or ONE row shared by every item.  Returns a dict: sk (n x 32), status (n: 0, 2, 32) and the records named in `want` -- chain,
        pk (pk_format), address (addr_format).  An item with a status has all-zero records.  device=True: everything stays on the GPU -- the inputs may be torch
        tensors on the engine's device, the dict holds torch uint8 tensors, and sk goes into ecdsa_sign_batch_device / eth_tx_sign_batch_device as it is (synchronises
        only as torch does)."""
        if device:
            return self._hd_derive_torch(False, parent_sk, parent_chain, path, pk_format, addr_format, want)
        fn = self._fn("plume_hd_derive_priv_batch")
        flags, n, depth, parent_sk, parent_chain, path = self._hd_shape(parent_sk, 32, parent_chain, path, "hd_derive_priv_batch")
        res = {"sk": np.zeros((n, 32), np.uint8), "status": np.zeros(n, np.uint8)}
        shape = {"chain": 32, "pk": ETH_PK_FORMATS[pk_format][1], "address": ETH_ADDR_FORMATS[addr_format][1]}
        for k in want:
            res[k] = np.zeros((n, shape[k]), np.uint8)
        self._chk(fn(self._ctx, flags, ETH_PK_FORMATS[pk_format][0], ETH_ADDR_FORMATS[addr_format][0], n, _ptr(parent_sk), _ptr(parent_chain), _ptr(path), depth,
                     _ptr(res["sk"]), _ptr(res.get("chain")), _ptr(res.get("pk")), _ptr(res.get("address")), _ptr(res["status"])), "plume_hd_derive_priv_batch")
        return res

    def hd_derive_pub_batch(self, parent_pk, parent_chain, path, pk_format="affine64", addr_format="raw20", want=("chain", "address"), device=False):
        """BIP-32 public derivation (plume_hd_derive_pub_batch): non-hardened indices only.  parent_pk in pk_format; the rest as hd_derive_priv_batch.  Returns a dict: pk
        (pk_format), status (n: 0, 2, 32, 64) and the records named in `want` -- chain, address."""
        if device:
            return self._hd_derive_torch(True, parent_pk, parent_chain, path, pk_format, addr_format, want)
        fn = self._fn("plume_hd_derive_pub_batch")
        flags, n, depth, parent_pk, parent_chain, path = self._hd_shape(parent_pk, ETH_PK_FORMATS[pk_format][1], parent_chain, path, "hd_derive_pub_batch")
        res = {"pk": np.zeros((n, ETH_PK_FORMATS[pk_format][1]), np.uint8), "status": np.zeros(n, np.uint8)}
        shape = {"chain": 32, "address": ETH_ADDR_FORMATS[addr_format][1]}
        for k in want:
            res[k] = np.zeros((n, shape[k]), np.uint8)
        self._chk(fn(self._ctx, flags, ETH_PK_FORMATS[pk_format][0], ETH_ADDR_FORMATS[addr_format][0], n, _ptr(parent_pk), _ptr(parent_chain), _ptr(path), depth,
                     _ptr(res["pk"]), _ptr(res.get("chain")), _ptr(res.get("address")), _ptr(res["status"])), "plume_hd_derive_pub_batch")
        return res

    def _hd_derive_torch(self, pub, parent, parent_chain, path, pk_format, addr_format, want):
        import torch
        dev = torch.device("cuda", self.device_id)
        width = ETH_PK_FORMATS[pk_format][1] if pub else 32

        def rows(a, w, dtype):
            t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32 if dtype is torch.int32 else np.uint8).view(np.int32 if dtype is torch.int32 else np.uint8))
            t = t.to(dev).contiguous()
            return t.reshape(1, -1) if t.ndim == 1 and w is None else (t if w is None else t.reshape(-1, w))
        parent, parent_chain, path = rows(parent, width, torch.uint8), rows(parent_chain, 32, torch.uint8), rows(path, None, torch.int32)
        if path.element_size() != 4:
            raise ValueError("path: a tensor of 4-byte indices")
        if len(parent) != len(parent_chain):
            raise ValueError(f"{len(parent)} parent keys and {len(parent_chain)} chain codes")
        n = max(len(parent), len(path))
        if len(parent) not in (1, n) or len(path) not in (1, n):
            raise ValueError(f"{len(parent)} parents and {len(path)} paths")
        flags = (HD_SHARED_PARENT if len(parent) == 1 and n > 1 else 0) | (HD_SHARED_PATH if len(path) == 1 and n > 1 else 0)
        z = lambda w: torch.zeros((n, w), dtype=torch.uint8, device=dev)  # noqa: E731
        res = {"status": torch.zeros(n, dtype=torch.uint8, device=dev)}
        if not pub:
            res["sk"] = z(32)
        shape = {"chain": 32, "pk": ETH_PK_FORMATS[pk_format][1], "address": ETH_ADDR_FORMATS[addr_format][1]}
        for k in tuple(want) + (("pk",) if pub else ()):
            res[k] = z(shape[k])
        # on a stream of its own between two waits: torch's default stream is the null stream, which the library takes to mean the context's stream -- and that one
        # is not ordered against the fills above or the caller's next use of the tensors
        cur = torch.cuda.current_stream(dev)
        st = torch.cuda.Stream(dev)
        st.wait_stream(cur)
        self.hd_derive_batch_device(pub, flags, n, parent, parent_chain, path, path.shape[1], res.get("sk"), res.get("chain"), res.get("pk"), res.get("address"),
                                    res["status"], pk_format, addr_format, stream=st)
        cur.wait_stream(st)
        for t in (parent, parent_chain, path, *res.values()):
            t.record_stream(st)
        return res

    @staticmethod
    def _kdf_shape(passwords, salt, bip39):
        """(n, pw, pw_off, flags, salt, salt_len) of a PBKDF2 call.  passwords: a list of bytes (str: NFKD, UTF-8), or (buf, off) as pack_messages returns them; salt:
        None or bytes -- ONE record shared by every item -- or an n x salt_len array"""
        pw, off = passwords if isinstance(passwords, tuple) else pack_messages([bip39_bytes(p) for p in passwords])
        n, pw, off = _ragged(pw, off)
        flags = KDF_BIP39 if bip39 else 0
        if salt is None or isinstance(salt, (str, bytes, bytearray, memoryview)):
            salt = np.frombuffer(bip39_bytes(salt or b""), dtype=np.uint8)
            return n, pw, off, flags | KDF_SHARED_SALT, salt, len(salt)
        salt = np.ascontiguousarray(salt, dtype=np.uint8)
        if salt.ndim != 2 or len(salt) != n:
            raise ValueError(f"salt: bytes shared by every item, or an n x salt_len array for the {n} items")
        return n, pw, off, flags, salt, salt.shape[1]

    def pbkdf2_sha512_batch(self, passwords, salt=None, iterations=2048, dklen=64, bip39=False, device=False):
        """PBKDF2-HMAC-SHA512, one output block, for a batch (plume_pbkdf2_sha512_batch).  passwords: a list of bytes of any length, or (buf, off) as pack_messages
        returns them; salt: None or bytes -- one record shared by every item -- or an n x salt_len array (salt_len <= 256); bip39: "mnemonic" goes in front of every
        salt on the device; 1 <= dklen <= 64.  Returns (out, status): n x dklen bytes and n status bytes, all 0 (the host form refuses unsound offsets as a whole).
        device=True: the device form on torch tensors of the engine's device, which the pair then holds -- an item of a caller's (buf, off) whose offsets decrease or
        reach past buf reports STATUS_KDF_BAD_INPUT (128) and an all-zero record; out goes into hd_master_batch_device as it is (synchronises only as torch does)."""
        n, pw, off, flags, salt, salt_len = self._kdf_shape(passwords, salt, bip39)
        if device:
            import torch
            dev = torch.device("cuda", self.device_id)
            up = lambda a: torch.from_numpy(np.array(a.view(np.int64) if a.dtype == np.uint64 else a)).to(dev)  # noqa: E731  (a copy: the caller's array may be read-only)
            pw, off, salt = up(pw), up(off), up(salt) if salt_len else None
            out, status = torch.zeros((n, int(dklen)), dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
            self._on_own_stream(dev, (pw, off, salt, out, status), lambda st: self.pbkdf2_sha512_batch_device(
                n, pw, off, pw.numel(), salt, salt_len, iterations, dklen, out, status, flags=flags, stream=st))
            return out, status
        fn = self._fn("plume_pbkdf2_sha512_batch")
        out, status = np.zeros((n, int(dklen)), np.uint8), np.zeros(n, np.uint8)
        self._chk(fn(self._ctx, flags, n, _ptr(pw), _ptr(off), _ptr(salt) if salt_len else None, int(salt_len), int(iterations), int(dklen), _ptr(out), _ptr(status)),
                  "plume_pbkdf2_sha512_batch")
        return out, status

    def bip39_seed_batch(self, mnemonics, passphrase="", device=False):
        """The BIP-39 seeds of mnemonic sentences: pbkdf2_sha512_batch with bip39=True, the passphrase as the one shared salt, 2048 iterations, 64 bytes.  str arguments
        are NFKD-normalised and UTF-8 encoded, bytes taken as given.  The word list is out of scope: a sentence is not checked against it.  Returns (seed, status)."""
        return self.pbkdf2_sha512_batch(mnemonics, bip39_bytes(passphrase), 2048, 64, bip39=True, device=device)

    def bip39_accounts(self, mnemonics, passphrase="", path="m/44'/60'/0'/0/0", device=False, want=("chain", "pk", "address"), pk_format="affine64", addr_format="raw20"):
        """Mnemonic sentences to account keys in one chain of device calls: bip39_seed_batch -> hd_master_batch_device -> hd_derive_priv_batch, with no host copy of a
        seed or a master key in between.  path: a BIP-32 path ("m/44'/60'/0'/0/0") or a row of indices shared by every item, or a list of n of either; ONE sentence with
        n paths gives n accounts of that wallet.  Returns the dict of hd_derive_priv_batch (sk, status, the records in `want`) as torch tensors on the device
        (device=True: sk goes into ecdsa_sign_batch_device / eth_tx_sign_batch_device as it is) or as numpy arrays.  status[i] is the first non-zero status of the three
        steps -- STATUS_KDF_BAD_INPUT (128), STATUS_HD_NO_KEY (32), 2 -- and every record of such an item is all zero: a zero seed would otherwise derive a
        real-looking key."""
        import torch
        from .plume import parse_path
        rows = [path] if isinstance(path, str) or (len(path) and isinstance(path[0], (int, np.integer))) else list(path)
        idx = np.array([parse_path(p) if isinstance(p, str) else [int(i) for i in p] for p in rows], dtype=np.uint32)
        seed, st0 = self.bip39_seed_batch(mnemonics, passphrase, device=True)
        n0, dev = len(st0), seed.device
        msk, mchain = torch.zeros((n0, 32), dtype=torch.uint8, device=dev), torch.zeros((n0, 32), dtype=torch.uint8, device=dev)
        st1 = torch.zeros(n0, dtype=torch.uint8, device=dev)
        if n0:
            self._on_own_stream(dev, (seed, msk, mchain, st1), lambda st: self.hd_master_batch_device(n0, seed, 64, msk, mchain, st1, stream=st))
        res = self._hd_derive_torch(False, msk, mchain, idx, pk_format, addr_format, want)
        before = torch.where(st0 != 0, st0, st1)                                # one row for a shared parent: it broadcasts over the items
        status = torch.where(before != 0, before, res["status"])
        keep = (status == 0).to(torch.uint8).reshape(-1, 1)
        res = {k: status if k == "status" else v * keep for k, v in res.items()}
        seed.zero_(); msk.zero_(); mchain.zero_()
        return res if device else {k: v.cpu().numpy() for k, v in res.items()}

    def _on_own_stream(self, dev, tensors, enqueue):
        """enqueue(stream) on a stream of its own between two waits: torch's default stream is the null stream, which the library takes to mean the context's stream --
        and that one is not ordered against the fills of `tensors` or the caller's next use of them"""
        import torch
        cur = torch.cuda.current_stream(dev)
        st = torch.cuda.Stream(dev)
        st.wait_stream(cur)
        enqueue(st)
        cur.wait_stream(st)
        for t in tensors:
            if t is not None:
                t.record_stream(st)

    @staticmethod
    def _merkle_items(leaf_format, addr_format, items, amounts):
        lf = MERKLE_LEAF_FORMATS[leaf_format]
        if addr_format == "eip55":
            af, W = ETH_ADDR_FORMATS[addr_format][0], 42                         # (the library refuses it: PLUME_ERR_ARG)
        else:
            af, W = ETH_ADDR_FORMATS[addr_format]
        W = 32 if lf == 0 else W
        items = np.ascontiguousarray(items, dtype=np.uint8)
        if items.size % W:
            raise ValueError(f"items: expected records of {W} bytes, got {items.size} bytes")
        n = items.size // W
        if lf == 2:
            if amounts is None:
                raise ValueError("the address_uint256 leaf needs amounts")
            if not (isinstance(amounts, np.ndarray) and amounts.dtype == np.uint8):
                amounts = np.frombuffer(b"".join(int(a).to_bytes(32, "big") for a in amounts), np.uint8)
            amounts = _np(amounts, 32, n, "amounts")
        else:
            amounts = None
        return lf, af, n, items, amounts

    def merkle_max_proof_len(self, n):
        """floor(log2(2n - 1)): the longest proof of a tree of n leaves (plume_merkle_max_proof_len)"""
        return int(self._fn("plume_merkle_max_proof_len")(int(n)) or 0)

    def merkle_leaf_batch(self, items, amounts=None, leaf_format="address", addr_format="raw20"):
        """The leaves of an OpenZeppelin StandardMerkleTree (plume_merkle_leaf_batch).  leaf_format "address": Keccak(Keccak(abi.encode(address))), the tree of
        ["address"]; "address_uint256": with amounts (integers, or n x 32 big-endian bytes), the tree of ["address", "uint256"]; "hash32": the items are the leaves.
        items: n x 20 ("raw20") or n x 64 ("record64": what eth_address_batch, ecdsa_recover_batch and eth_tx_sender_batch write).  Returns (leaf n x 32, status):
        MERKLE_MATCH, or MERKLE_INVALID and a zero leaf for a record64 whose first 44 bytes are not zero."""
        fn = self._fn("plume_merkle_leaf_batch")
        lf, af, n, items, amounts = self._merkle_items(leaf_format, addr_format, items, amounts)
        leaf, status = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
        self._chk(fn(self._ctx, lf, af, n, _ptr(items), _ptr(amounts), _ptr(leaf), _ptr(status)), "plume_merkle_leaf_batch")
        return leaf, status

    def merkle_tree_build(self, leaves, sort=True):
        """(tree (2n - 1) x 32, leaf_pos n uint32) of n >= 1 leaves of 32 bytes (plume_merkle_tree_build): tree[0] is the root, the leaves sit at the end in reverse,
        sorted by (bytes, input index) when sort is set; leaf_pos[j] is the tree index of input leaf j."""
        fn = self._fn("plume_merkle_tree_build")
        leaves = np.ascontiguousarray(leaves, dtype=np.uint8)
        if leaves.size % 32:
            raise ValueError(f"leaves: expected records of 32 bytes, got {leaves.size} bytes")
        n = leaves.size // 32
        tree, leaf_pos = np.zeros((max(2 * n - 1, 0), 32), np.uint8), np.zeros(n, np.uint32)
        self._chk(fn(self._ctx, MERKLE_SORT_LEAVES if sort else 0, n, _ptr(leaves), _ptr(tree), _ptr(leaf_pos)), "plume_merkle_tree_build")
        return tree, leaf_pos

    def merkle_proof_batch(self, tree, pos, depth=None):
        """The proofs of the tree indices pos (plume_merkle_proof_batch): (proof m x depth x 32, proof_len m).  depth defaults to the longest proof of the tree; unused
        slots are zero; an index outside the tree, or a proof longer than depth, gives MERKLE_BAD_PROOF and zero slots."""
        fn = self._fn("plume_merkle_proof_batch")
        tree = np.ascontiguousarray(tree, dtype=np.uint8)
        n = (tree.size // 32 + 1) // 2
        if tree.size % 32 or tree.size // 32 != 2 * n - 1:
            raise ValueError(f"tree: expected 2n - 1 nodes of 32 bytes, got {tree.size} bytes")
        pos = np.ascontiguousarray(pos, dtype=np.uint32)
        depth = self.merkle_max_proof_len(n) if depth is None else int(depth)
        proof, proof_len = np.zeros((len(pos), depth, 32), np.uint8), np.zeros(len(pos), np.uint8)
        self._chk(fn(self._ctx, n, _ptr(tree), len(pos), _ptr(pos), depth, _ptr(proof) if depth else None, _ptr(proof_len)), "plume_merkle_proof_batch")
        return proof, proof_len

    def merkle_verify_batch(self, items, proof, proof_len, root, amounts=None, leaf_format="address", addr_format="raw20"):
        """MerkleProof.verify for every item against one root (plume_merkle_verify_batch).  items and amounts as merkle_leaf_batch takes them (the leaf is computed on the
        GPU); proof: m x depth x 32, proof_len: m bytes.  Returns status: MERKLE_MATCH, MERKLE_MISMATCH, or MERKLE_INVALID (an invalid item, or proof_len above depth)."""
        fn = self._fn("plume_merkle_verify_batch")
        lf, af, m, items, amounts = self._merkle_items(leaf_format, addr_format, items, amounts)
        proof = np.ascontiguousarray(proof, dtype=np.uint8)
        if m == 0 or proof.size % (32 * m):
            if m or proof.size:
                raise ValueError(f"proof: expected {m} x depth x 32 bytes, got {proof.size} bytes")
        depth = proof.size // (32 * m) if m else 0
        proof_len = _np(proof_len, 1, m, "proof_len")
        root = _np(root, 32, 1, "root")
        status = np.zeros(m, np.uint8)
        self._chk(fn(self._ctx, lf, af, m, _ptr(items), _ptr(amounts), depth, _ptr(proof) if depth else None, _ptr(proof_len), _ptr(root), _ptr(status)),
                  "plume_merkle_verify_batch")
        return status

    def merkle_tree(self, items, amounts=None, sort=True, leaf_format=None, addr_format="raw20"):
        """A MerkleTree over leaves (n x 32 bytes: leaf_format None or "hash32") or over addresses (leaf_format "address", or "address_uint256" when amounts are given):
        the leaves, the tree and its proofs come from the GPU.  Raises ValueError when an address record is invalid."""
        if leaf_format is None:
            leaf_format = "address_uint256" if amounts is not None else "hash32" if len(items) and len(items[0]) == 32 else "address"
        if not isinstance(items, np.ndarray):
            items = np.frombuffer(b"".join(bytes(x) for x in items), np.uint8)
        if leaf_format == "hash32":
            leaves = np.ascontiguousarray(items, dtype=np.uint8).reshape(-1, 32)
        else:
            leaves, st = self.merkle_leaf_batch(items, amounts, leaf_format, addr_format)
            if (st != MERKLE_MATCH).any():
                raise ValueError(f"item {int(np.flatnonzero(st != MERKLE_MATCH)[0])} is no address record")
        tree, leaf_pos = self.merkle_tree_build(leaves, sort)
        return MerkleTree(self, tree, leaf_pos, leaf_format, addr_format)

    def verify_batch_sec1(self, version, msgs, msg_off, pk33, nullifier33, c, s, r_point33=None, hashed_to_curve_r33=None):
        """verify with 33-byte SEC1-compressed points (decompressed and validated on the GPU)"""
        n, msgs, msg_off = _ragged(msgs, msg_off)
        pk33, nullifier33, c, s = _np(pk33, 33, n, "pk33"), _np(nullifier33, 33, n, "nullifier33"), _np(c, 32, n, "c"), _np(s, 32, n, "s")
        if version == 1:
            if r_point33 is None or hashed_to_curve_r33 is None:
                raise ValueError("V1 verification needs r_point and hashed_to_curve_r")
            r_point33, hashed_to_curve_r33 = _np(r_point33, 33, n, "r_point33"), _np(hashed_to_curve_r33, 33, n, "hashed_to_curve_r33")
        else:
            r_point33 = hashed_to_curve_r33 = None
        ok = np.zeros(n, dtype=np.uint8)
        self._chk(self._lib.plume_verify_batch_sec1(self._ctx, int(version), n, _ptr(msgs), _ptr(msg_off), _ptr(pk33), _ptr(nullifier33), _ptr(c), _ptr(s),
                                                    _ptr(r_point33), _ptr(hashed_to_curve_r33), _ptr(ok)), "plume_verify_batch_sec1")
        return ok

    def sign_batch(self, version, msgs, msg_off, sk, r, pk_in=None, out=None):
        """out: optional dict of preallocated arrays (pk, nullifier, c, s, r_point, hashed_to_curve_r, status), e.g. page-locked ones"""
        n, msgs, msg_off = _ragged(msgs, msg_off)
        sk, r = _np(sk, 32, n, "sk"), _np(r, 32, n, "r")
        pk_in = None if pk_in is None else _np(pk_in, 64, n, "pk_in")
        o = _sign_outputs(n, 64, out)
        self._chk(self._lib.plume_sign_batch(self._ctx, int(version), n, _ptr(msgs), _ptr(msg_off), _ptr(sk), _ptr(r), _ptr(pk_in), *(_ptr(o[k]) for k in _SIGN_OUTPUTS)),
                  "plume_sign_batch")
        return o

    def sign_batch_rfc6979(self, version, msgs, msg_off, sk, aux=None, pk_in=None, out=None):
        """sign_batch with each nonce derived on the GPU by RFC 6979 (include/plume_hip.h, plume_sign_batch_rfc6979): h1 = SHA-256("PLUME-RFC6979" || version || mode ||
        pk_in || msg), x = sk; aux (n x 32 bytes, optional) is the hedging input of RFC 6979 section 3.6.  The nonces never reach host memory.  Same outputs as sign_batch."""
        fn = self._fn("plume_sign_batch_rfc6979")
        n, msgs, msg_off = _ragged(msgs, msg_off)
        sk = _np(sk, 32, n, "sk")
        aux = None if aux is None else _np(aux, 32, n, "aux")
        pk_in = None if pk_in is None else _np(pk_in, 64, n, "pk_in")
        o = _sign_outputs(n, 64, out)
        self._chk(fn(self._ctx, int(version), n, _ptr(msgs), _ptr(msg_off), _ptr(sk), _ptr(aux), _ptr(pk_in), *(_ptr(o[k]) for k in _SIGN_OUTPUTS)), "plume_sign_batch_rfc6979")
        return o

    def sign_batch_sec1(self, version, msgs, msg_off, sk, r, pk_in=None):
        """sign_batch with pk, nullifier, r_point, hashed_to_curve_r as 33-byte SEC1-compressed records"""
        n, msgs, msg_off = _ragged(msgs, msg_off)
        sk, r = _np(sk, 32, n, "sk"), _np(r, 32, n, "r")
        pk_in = None if pk_in is None else _np(pk_in, 64, n, "pk_in")
        o = _sign_outputs(n, 33)
        self._chk(self._lib.plume_sign_batch_sec1(self._ctx, int(version), n, _ptr(msgs), _ptr(msg_off), _ptr(sk), _ptr(r), _ptr(pk_in), *(_ptr(o[k]) for k in _SIGN_OUTPUTS)),
                  "plume_sign_batch_sec1")
        return o

    def hash_to_curve_batch(self, msgs, msg_off, pk=None):
        n, msgs, msg_off = _ragged(msgs, msg_off)
        pk = None if pk is None else _np(pk, 64, n, "pk")
        h = np.zeros((n, 64), dtype=np.uint8)
        self._chk(self._lib.plume_hash_to_curve_batch(self._ctx, n, _ptr(msgs), _ptr(msg_off), _ptr(pk), _ptr(h)), "plume_hash_to_curve_batch")
        return h

    def h2c_intermediates_batch(self, msgs, msg_off, pk=None, registers=False):
        """circuit witness hints from the GPU hash_to_curve: dict u (n,2,·), mapped (n,4,·), q (n,4,·), h (n,2,·); values are 32
        big-endian bytes (uint8, last axis 32) or, with registers=True, 4 little-endian 64-bit registers (uint64, last axis 4)"""
        n, msgs, msg_off = _ragged(msgs, msg_off)
        pk = None if pk is None else _np(pk, 64, n, "pk")
        o = {k: np.zeros((n, w, 32), dtype=np.uint8) for k, w in [("u", 2), ("mapped", 4), ("q", 4), ("h", 2)]}
        self._chk(self._lib.plume_h2c_intermediates_batch(self._ctx, n, _ptr(msgs), _ptr(msg_off), _ptr(pk), 1 if registers else 0, _ptr(o["u"]), _ptr(o["mapped"]),
                                                          _ptr(o["q"]), _ptr(o["h"])), "plume_h2c_intermediates_batch")
        if registers:
            o = {k: v.view(np.uint64) for k, v in o.items()}
        return o

    def h2c_hints_batch(self, msgs, msg_off, pk=None, registers=False):
        """the circuit's square-root hints (UNPINNED definitions, include/plume_hip.h): dict q0_gx1_sqrt, q0_gx2_sqrt, q0_y_pos, q1_... -> (n, 32) bytes or (n, 4) uint64 registers"""
        n, msgs, msg_off = _ragged(msgs, msg_off)
        pk = None if pk is None else _np(pk, 64, n, "pk")
        out = np.zeros((n, 6, 32), dtype=np.uint8)
        self._chk(self._lib.plume_h2c_hints_batch(self._ctx, n, _ptr(msgs), _ptr(msg_off), _ptr(pk), 1 if registers else 0, _ptr(out)), "plume_h2c_hints_batch")
        names = ["q0_gx1_sqrt", "q0_gx2_sqrt", "q0_y_pos", "q1_gx1_sqrt", "q1_gx2_sqrt", "q1_y_pos"]
        return {nm: (np.ascontiguousarray(out[:, k]).view(np.uint64) if registers else np.ascontiguousarray(out[:, k])) for k, nm in enumerate(names)}

    def scalars_to_sec1_der_batch(self, scalars):
        """SecretKey::from(scalar).to_sec1_der() for a batch (javascript/src/lib.rs:98-110): (n, 109) records incl. the public key scalar*G computed on the GPU,
        and a status array (2 = scalar outside [1, n-1], record zeroed)"""
        scalars = np.ascontiguousarray(scalars, dtype=np.uint8).reshape(-1, 32)
        n = len(scalars)
        der, status = np.zeros((n, 109), dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        self._chk(self._lib.plume_scalars_to_sec1_der_batch(self._ctx, n, _ptr(scalars), _ptr(der), _ptr(status)), "plume_scalars_to_sec1_der_batch")
        return der, status

    def sec1_der_to_scalars(self, der109):
        """SecretKey::from_sec1_der with the reference's semantics: structure, scalar range and public key == scalar * G (recomputed on the GPU) -> (scalars (n, 32), ok (n,))"""
        d = np.ascontiguousarray(der109, dtype=np.uint8).reshape(-1, 109)
        sc, ok = np.zeros((len(d), 32), dtype=np.uint8), np.zeros(len(d), dtype=np.uint8)
        self._chk(self._lib.plume_sec1_der_to_scalars_checked(self._ctx, len(d), _ptr(d), _ptr(sc), _ptr(ok)), "plume_sec1_der_to_scalars_checked")
        return sc, ok

    def nullifier_first_occurrence(self, nullifier, live=None, ids=None):
        """first[i] = 1 iff item i is live and holds the smallest id (default: position) among the live items with the same 64-byte
        nullifier; returns (first uint8[n], number of ones)"""
        nullifier = np.ascontiguousarray(nullifier, dtype=np.uint8).reshape(-1, 64)
        n = len(nullifier)
        live = None if live is None else np.ascontiguousarray(live, dtype=np.uint8).reshape(n)
        ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint64).reshape(n)
        first = np.zeros(n, dtype=np.uint8)
        cnt = C.c_uint64(0)
        self._chk(self._lib.plume_nullifier_first_occurrence(self._ctx, n, _ptr(nullifier), _ptr(live), _ptr(ids), _ptr(first), C.byref(cnt)),
                  "plume_nullifier_first_occurrence")
        return first, int(cnt.value)

    # ------------------------------------------------------------------ device-resident API (torch uint8 tensors on this GPU)
    @staticmethod
    def _dp(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def verify_batch_device(self, version, n, msgs, msg_off, msgs_bytes, pk, nullifier, c, s, r_point, hashed_to_curve_r, ok, stream=None):
        """all tensors on cuda:<device_id>; enqueues on `stream` (torch.cuda.Stream or None = current stream); does not synchronise"""
        d = self._dp
        self._enqueue("plume_verify_batch_device", stream, int(version), int(n), d(msgs), d(msg_off), int(msgs_bytes), d(pk), d(nullifier), d(c), d(s),
                      d(r_point), d(hashed_to_curve_r), d(ok))

    def recover_batch_device(self, version, n, msgs, msg_off, msgs_bytes, pk, nullifier, c, s, r_point, hashed_to_curve_r, hashed_to_curve, status,
                             fmt=RECOVER_FMT_AFFINE64, stream=None):
        """the device form of recover_batch on torch tensors; each of the four outputs may be None (at least one is not); enqueues on `stream` (None = current
        stream); does not synchronise"""
        d = self._dp
        self._enqueue("plume_recover_batch_device", stream, int(version), int(fmt), int(n), d(msgs), d(msg_off), int(msgs_bytes), d(pk), d(nullifier), d(c), d(s),
                      d(r_point), d(hashed_to_curve_r), d(hashed_to_curve), d(status))

    def eth_address_batch_device(self, n, pk, expect, address, status, pk_format="affine64", addr_format="raw20", stream=None):
        """the device form of eth_address_batch on torch tensors; expect may be None, and one of address and status; enqueues on `stream` (None = current stream); does
        not synchronise"""
        d = self._dp
        self._enqueue("plume_eth_address_batch_device", stream, ETH_PK_FORMATS[pk_format][0], ETH_ADDR_FORMATS[addr_format][0], int(n), d(pk), d(expect), d(address), d(status))

    def ecdsa_recover_batch_device(self, n, hash, r, s, v, expect, pk, address, status, pk_format="affine64", addr_format="raw20", low_s=False, stream=None):
        """the device form of ecdsa_recover_batch on torch tensors; expect may be None, and any two of pk, address and status; enqueues on `stream` (None = current
        stream); does not synchronise"""
        d = self._dp
        self._enqueue("plume_ecdsa_recover_batch_device", stream, ECDSA_LOW_S if low_s else 0, ETH_PK_FORMATS[pk_format][0], ETH_ADDR_FORMATS[addr_format][0], int(n),
                      d(hash), d(r), d(s), d(v), d(expect), d(pk), d(address), d(status))

    def eth_message_hash_batch_device(self, n, msgs, msg_off, msgs_bytes, hash32, mode="eip191", stream=None):
        """the device form of eth_message_hash_batch on torch tensors (msg_off: n + 1 uint64 offsets; msgs and hash32 at any byte offset); one kernel on `stream`
        (None = current stream); does not synchronise"""
        d = self._dp
        self._enqueue("plume_eth_message_hash_batch_device", stream, int(ETH_HASH_MODES.get(mode, mode)), int(n), d(msgs), d(msg_off), int(msgs_bytes), d(hash32))

    def eth_tx_parse_batch_device(self, n, txs, tx_off, txs_bytes, hash32, r, s, v, chain_id=None, tx_type=None, status=None, stream=None):
        """the device form of eth_tx_parse_batch on torch tensors (tx_off: n + 1 uint64 offsets; chain_id: n 8-byte words; the byte arrays at any byte offset; chain_id,
        tx_type and status may be None); one kernel on `stream` (None = current stream); does not synchronise"""
        d = self._dp
        self._enqueue("plume_eth_tx_parse_batch_device", stream, int(n), d(txs), d(tx_off), int(txs_bytes), d(hash32), d(r), d(s), d(v), d(chain_id), d(tx_type), d(status))

    def eth_tx_sender_batch_device(self, n, txs, tx_off, txs_bytes, expect, pk, address, chain_id, tx_type, status, pk_format="affine64", addr_format="raw20", low_s=True,
                                   stream=None):
        """the device form of eth_tx_sender_batch on torch tensors; expect, chain_id and tx_type may be None, and any two of pk, address and status; enqueues on `stream`
        (None = current stream); does not synchronise"""
        d = self._dp
        self._enqueue("plume_eth_tx_sender_batch_device", stream, ECDSA_LOW_S if low_s else 0, ETH_PK_FORMATS[pk_format][0], ETH_ADDR_FORMATS[addr_format][0], int(n),
                      d(txs), d(tx_off), int(txs_bytes), d(expect), d(pk), d(address), d(chain_id), d(tx_type), d(status))

    def eth_tx_sign_batch_device(self, n, txs, tx_off, txs_bytes, sk, aux, out, out_bytes, out_len, status, hash32=None, r=None, s=None, v=None, chain_id=None, tx_type=None,
                                 stream=None):
        """the device form of eth_tx_sign_batch on torch tensors (tx_off: n + 1 uint64 offsets; out: the slots, out_bytes of them; out_len: n 4-byte words; chain_id: n
        8-byte words; the byte arrays at any byte offset; aux and the records may be None); enqueues on `stream` (None = current stream); does not synchronise"""
        d = self._dp
        self._enqueue("plume_eth_tx_sign_batch_device", stream, 0, int(n), d(txs), d(tx_off), int(txs_bytes), d(sk), d(aux), d(out), int(out_bytes), d(out_len),
                      d(hash32), d(r), d(s), d(v), d(chain_id), d(tx_type), d(status))

    def hd_master_batch_device(self, n, seed, seed_len, sk, chain, status, stream=None):
        """the device form of hd_master_batch on torch tensors; one kernel on `stream` (None = current stream); does not synchronise"""
        d = self._dp
        self._enqueue("plume_hd_master_batch_device", stream, int(n), d(seed), int(seed_len), d(sk), d(chain), d(status))

    def hd_derive_batch_device(self, pub, flags, n, parent, parent_chain, path, depth, child_sk, child_chain, child_pk, address, status, pk_format="affine64",
                               addr_format="raw20", stream=None):
        """the device forms of hd_derive_priv_batch (pub False: parent is sk, child_sk required) and hd_derive_pub_batch (pub True: parent is pk, child_sk ignored, child_pk
        required) on torch tensors; path: n x depth 4-byte indices (one row with HD_SHARED_PATH); the optional records may be None; enqueues on `stream` (None = current
        stream); does not synchronise.  child_sk is what ecdsa_sign_batch_device and eth_tx_sign_batch_device take as sk."""
        d = self._dp
        head = (int(flags), ETH_PK_FORMATS[pk_format][0], ETH_ADDR_FORMATS[addr_format][0], int(n), d(parent), d(parent_chain), d(path), int(depth))
        if pub:
            self._enqueue("plume_hd_derive_pub_batch_device", stream, *head, d(child_pk), d(child_chain), d(address), d(status))
        else:
            self._enqueue("plume_hd_derive_priv_batch_device", stream, *head, d(child_sk), d(child_chain), d(child_pk), d(address), d(status))

    def pbkdf2_sha512_batch_device(self, n, pw, pw_off, pw_bytes, salt, salt_len, iterations, dklen, out, status, flags=0, stream=None):
        """the device form of pbkdf2_sha512_batch on torch tensors (pw_off: n + 1 uint64 offsets into the pw_bytes bytes of pw; salt: salt_len bytes per item, one record
        with KDF_SHARED_SALT, None when salt_len is 0; out: n x dklen bytes; flags: KDF_BIP39 | KDF_SHARED_SALT); enqueues on `stream` (None = current stream); does not
        synchronise"""
        d = self._dp
        self._enqueue("plume_pbkdf2_sha512_batch_device", stream, int(flags), int(n), d(pw), d(pw_off), int(pw_bytes), d(salt), int(salt_len), int(iterations), int(dklen),
                      d(out), d(status))

    def merkle_leaf_batch_device(self, n, items, amounts, leaf32, status, leaf_format="address", addr_format="raw20", stream=None):
        """the device form of merkle_leaf_batch on torch tensors; amounts (n x 32 big-endian bytes) and status may be None; one kernel on `stream` (None = current
        stream); does not synchronise"""
        d = self._dp
        self._enqueue("plume_merkle_leaf_batch_device", stream, MERKLE_LEAF_FORMATS[leaf_format], ETH_ADDR_FORMATS[addr_format][0], int(n), d(items), d(amounts), d(leaf32),
                      d(status))

    def merkle_tree_build_device(self, n, leaf32, tree, leaf_pos, sort=True, stream=None):
        """the device form of merkle_tree_build on torch tensors (tree: (2n - 1) x 32 bytes; leaf_pos: n 4-byte words, or None); enqueues on `stream` (None = current
        stream); does not synchronise"""
        d = self._dp
        self._enqueue("plume_merkle_tree_build_device", stream, MERKLE_SORT_LEAVES if sort else 0, int(n), d(leaf32), d(tree), d(leaf_pos))

    def merkle_proof_batch_device(self, n, tree, m, pos, depth, proof, proof_len, stream=None):
        """the device form of merkle_proof_batch on torch tensors (pos: m 4-byte words; proof: m x depth x 32 bytes; proof_len: m bytes); one kernel on `stream` (None =
        current stream); does not synchronise"""
        d = self._dp
        self._enqueue("plume_merkle_proof_batch_device", stream, int(n), d(tree), int(m), d(pos), int(depth), d(proof), d(proof_len))

    def merkle_verify_batch_device(self, m, items, amounts, depth, proof, proof_len, root32, status, leaf_format="address", addr_format="raw20", stream=None):
        """the device form of merkle_verify_batch on torch tensors; amounts may be None; one kernel on `stream` (None = current stream); does not synchronise"""
        d = self._dp
        self._enqueue("plume_merkle_verify_batch_device", stream, MERKLE_LEAF_FORMATS[leaf_format], ETH_ADDR_FORMATS[addr_format][0], int(m), d(items), d(amounts), int(depth),
                      d(proof), d(proof_len), d(root32), d(status))

    def ecdsa_sign_batch_device(self, n, hash, sk, aux, r, s, v, status, v27=False, stream=None):
        """the device form of ecdsa_sign_batch on torch tensors; aux may be None; enqueues on `stream` (None = current stream); does not synchronise"""
        d = self._dp
        self._enqueue("plume_ecdsa_sign_batch_device", stream, ECDSA_SIGN_V27 if v27 else 0, int(n), d(hash), d(sk), d(aux), d(r), d(s), d(v), d(status))

    def verify_non_zk_batch_device(self, version, n, msgs, msg_off, msgs_bytes, pk, nullifier, s, r_point, hashed_to_curve_r, digest_private, ok, stream=None):
        d = self._dp
        self._enqueue("plume_verify_non_zk_batch_device", stream, int(version), int(n), d(msgs), d(msg_off), int(msgs_bytes), d(pk), d(nullifier), d(s), d(r_point),
                      d(hashed_to_curve_r), d(digest_private), d(ok))

    def aggregate_check_device(self, version, mode, n, msgs, msg_off, msgs_bytes, pk, nullifier, c, s, r_point, hashed_to_curve_r, seed, index_base, hash_ok, result, stream=None):
        """device tensors; seed: 32 host bytes; hash_ok: uint8[n] or None; result: uint8[72] (parse_aggregate_record after synchronising)"""
        d = self._dp
        sd = np.frombuffer(bytes(seed), dtype=np.uint8).copy()
        self._enqueue("plume_aggregate_check_device", stream, int(version), int(mode), int(n), d(msgs), d(msg_off), int(msgs_bytes), d(pk), d(nullifier), d(c), d(s), d(r_point),
                      d(hashed_to_curve_r), _ptr(sd), int(index_base), d(hash_ok), d(result))

    def verify_batch_sec1_device(self, version, n, msgs, msg_off, msgs_bytes, pk33, nullifier33, c, s, r_point33, hashed_to_curve_r33, ok, stream=None):
        d = self._dp
        self._enqueue("plume_verify_batch_sec1_device", stream, int(version), int(n), d(msgs), d(msg_off), int(msgs_bytes), d(pk33), d(nullifier33), d(c), d(s),
                      d(r_point33), d(hashed_to_curve_r33), d(ok))

    def sign_batch_device(self, version, n, msgs, msg_off, msgs_bytes, sk, r, pk_in, pk, nullifier, c, s, r_point, hashed_to_curve_r, status, stream=None):
        d = self._dp
        self._enqueue("plume_sign_batch_device", stream, int(version), int(n), d(msgs), d(msg_off), int(msgs_bytes), d(sk), d(r), d(pk_in), d(pk),
                      d(nullifier), d(c), d(s), d(r_point), d(hashed_to_curve_r), d(status))

    def sign_batch_rfc6979_device(self, version, n, msgs, msg_off, msgs_bytes, sk, aux, pk_in, pk, nullifier, c, s, r_point, hashed_to_curve_r, status, stream=None):
        """the device form of sign_batch_rfc6979 on torch tensors (aux, pk_in: None or tensors); enqueues on `stream` (None = current stream); does not synchronise"""
        d = self._dp
        self._enqueue("plume_sign_batch_rfc6979_device", stream, int(version), int(n), d(msgs), d(msg_off), int(msgs_bytes), d(sk), d(aux), d(pk_in), d(pk), d(nullifier),
                      d(c), d(s), d(r_point), d(hashed_to_curve_r), d(status))

    def nullifier_first_occurrence_device(self, n, nullifier, live, ids, first, n_unique=None, stream=None):
        """tensors on cuda:<device_id> (nullifier n x 64 uint8, live / first uint8[n] or None, ids int64/uint64[n] or None, n_unique one 64-bit word or None)"""
        d = self._dp
        self._enqueue("plume_nullifier_first_occurrence_device", stream, int(n), d(nullifier), d(live), d(ids), d(first), d(n_unique))

    # ------------------------------------------------------------------ persistent nullifier set
    def nullifier_set(self, reserve=0):
        """a GPU-resident set of 64-byte nullifiers that persists across calls (include/plume_hip.h, plume_nullset_*), on this context's device
        (the first one of a multi-device engine); see NullifierSet"""
        return NullifierSet(self, reserve)

    # ------------------------------------------------------------------ measurement
    def set_stage_timing(self, on):
        """per-stage timing events inside the device pipelines (plume_set_stage_timing): OFF by default since library 0.5 -- an event between two kernels costs ~6 us of idle
        GPU, five or six per call.  Env PLUME_STAGE_TIMES=1 turns it on for new contexts."""
        fn = getattr(self._lib, "plume_set_stage_timing", None)
        if fn is None:
            return                                   # an older library (PLUME_HIP_LIB): always on
        self._chk(fn(self._ctx, 1 if on else 0), "plume_set_stage_timing")

    def last_stage_times(self):
        """(stage, ms) of the last device-resident call; needs set_stage_timing(True) (or PLUME_STAGE_TIMES=1) BEFORE that call"""
        cap = 512
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        k = self._lib.plume_last_stage_times(self._ctx, names, ms, cap)
        if k < 0:
            raise PlumeHipError(f"plume_last_stage_times failed ({k}): {self._lib.plume_last_error().decode()}")
        return [(names[i].decode(), float(ms[i])) for i in range(min(k, cap))]

    def last_redo_tasks(self):
        """multi-scalar tasks of the last verify call that met p == +-q in an unchecked addition and were redone with checked additions (0 for honest batches).
        Raises PlumeHipError once an ECDSA-family call (ecdsa_recover_batch, eth_tx_sender_batch, a self-checked ecdsa_sign_batch / eth_tx_sign_batch) has reused the redo
        list on the context or lane this reads: the count would be another family's.  The next verify call re-arms it."""
        c = C.c_uint64(0)
        self._chk(self._lib.plume_last_redo_tasks(self._ctx, C.byref(c)), "plume_last_redo_tasks")
        return int(c.value)

    def microbench(self, kind, iters=4096):
        v = self._lib.plume_microbench(self._ctx, int(kind), int(iters))
        if v <= 0:
            raise PlumeHipError(f"plume_microbench failed: {self._lib.plume_last_error().decode()}")
        return float(v)

    def microbench_ticks(self):
        ms = C.c_float()
        t = self._lib.plume_microbench_last_ticks(C.byref(ms))
        return float(t), float(ms.value)


class MerkleTree:
    """A tree built by Engine.merkle_tree: .root (32 bytes), .tree ((2n - 1) x 32 uint8), .leaf_pos (n uint32: the tree index of input item j), .n, and
    .proofs(indices): the proofs of the INPUT items `indices` (all of them by default) as (proof m x depth x 32, proof_len m), from the GPU."""

    def __init__(self, engine, tree, leaf_pos, leaf_format, addr_format):
        self.engine, self.tree, self.leaf_pos, self.leaf_format, self.addr_format = engine, tree, leaf_pos, leaf_format, addr_format
        self.n = len(leaf_pos)
        self.root = tree[0].tobytes()
        self.depth = engine.merkle_max_proof_len(self.n)

    def proofs(self, indices=None):
        idx = np.arange(self.n) if indices is None else np.asarray(indices, dtype=np.int64)
        return self.engine.merkle_proof_batch(self.tree, self.leaf_pos[idx], self.depth)

    def proof(self, index):
        """the proof of input item `index` as a list of 32-byte strings"""
        p, ln = self.proofs([index])
        return [p[0, s].tobytes() for s in range(int(ln[0]))]


def _version(lib):
    return tuple(int(x) for x in lib.plume_version().decode().split()[1].split(".")[:2])


class NullifierSet:
    """A set S of distinct 64-byte records on the GPU that persists across calls: the step after `verify` for a consumer of a stream of batches,
    which must accept ONE signature per nullifier, ever.  insert(nullifier, live, ids) -> (fresh, n_fresh): fresh[i] = 1 iff the item is live, its
    record was not in S before the call and no live item of the call with the same record has a smaller id (default: position); S then holds every
    live record.  contains / export / clear / reserve / len; the *_device forms take torch tensors on the set's device and do not synchronise
    (the set orders its operations itself, whatever streams they are issued on).  One host thread at a time.  May outlive its Engine."""

    def __init__(self, engine, reserve=0):
        lib = engine._lib
        since, what = GROUPS["nullset"]
        if getattr(lib, "plume_nullset_create", None) is None or _version(lib) < since:
            raise PlumeHipError(f"{lib.plume_version().decode()} has no {what}: it needs plume_hip >= {since[0]}.{since[1]} (rebuild: make -C zk-nullifier-sig_amd/csrc)")
        self._lib = lib
        self.device_id = engine.device_id
        self._h = C.c_void_p()
        rc = lib.plume_nullset_create(engine._ctx, int(reserve), C.byref(self._h))
        if rc != 0:
            self._h = None
            raise PlumeHipError(f"plume_nullset_create failed ({rc}): {lib.plume_last_error().decode()}")

    def _chk(self, rc, what):
        if rc != 0:
            raise PlumeHipError(f"{what} failed ({rc}): {self._lib.plume_last_error().decode()}")

    def _handle(self):
        if not self._h:
            raise PlumeHipError("the nullifier set is closed")
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.plume_nullset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _size(self):
        size, cap = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._lib.plume_nullset_size(self._handle(), C.byref(size), C.byref(cap)), "plume_nullset_size")
        return int(size.value), int(cap.value)

    def __len__(self):
        return self._size()[0]

    @property
    def capacity(self):
        """slots of the table (a power of two, at least twice the size)"""
        return self._size()[1]

    def reserve(self, items):
        self._chk(self._lib.plume_nullset_reserve(self._handle(), int(items)), "plume_nullset_reserve")

    def clear(self):
        self._chk(self._lib.plume_nullset_clear(self._handle()), "plume_nullset_clear")

    def insert(self, nullifier, live=None, ids=None):
        """numpy in / out: (fresh uint8[n], number of fresh items)"""
        nullifier = np.ascontiguousarray(nullifier, dtype=np.uint8).reshape(-1, 64)
        n = len(nullifier)
        live = None if live is None else np.ascontiguousarray(live, dtype=np.uint8).reshape(n)
        ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint64).reshape(n)
        fresh = np.zeros(n, dtype=np.uint8)
        cnt = C.c_uint64(0)
        self._chk(self._lib.plume_nullset_insert(self._handle(), n, _ptr(nullifier), _ptr(live), _ptr(ids), _ptr(fresh), C.byref(cnt)), "plume_nullset_insert")
        return fresh, int(cnt.value)

    def contains(self, nullifier):
        """numpy in / out: found uint8[n]"""
        nullifier = np.ascontiguousarray(nullifier, dtype=np.uint8).reshape(-1, 64)
        found = np.zeros(len(nullifier), dtype=np.uint8)
        self._chk(self._lib.plume_nullset_contains(self._handle(), len(nullifier), _ptr(nullifier), _ptr(found)), "plume_nullset_contains")
        return found

    def export(self):
        """every record, uint8[len, 64], in no particular order"""
        cnt = C.c_uint64(0)
        self._chk(self._lib.plume_nullset_export(self._handle(), 0, None, C.byref(cnt)), "plume_nullset_export")
        out = np.zeros((int(cnt.value), 64), dtype=np.uint8)
        if len(out):
            self._chk(self._lib.plume_nullset_export(self._handle(), len(out), _ptr(out), C.byref(cnt)), "plume_nullset_export")
        return out[:int(cnt.value)]

    def _stream(self, stream):
        import torch
        return (stream or torch.cuda.current_stream(self.device_id)).cuda_stream

    def insert_device(self, n, nullifier, live, ids, fresh, n_fresh=None, stream=None):
        """tensors on the set's device (nullifier n x 64 uint8, live / fresh uint8[n] or None, ids int64/uint64[n] or None, n_fresh one 64-bit word or None);
        enqueued on `stream` (torch.cuda.Stream or None = the current stream); does not synchronise.  torch's default stream has the handle 0, which the library
        reads as "the set's own stream": to chain an insert behind other work (a verify_batch_device), issue both on one non-default torch stream"""
        d = Engine._dp
        self._chk(self._lib.plume_nullset_insert_device(self._handle(), int(n), d(nullifier), d(live), d(ids), d(fresh), d(n_fresh), C.c_void_p(self._stream(stream))),
                  "plume_nullset_insert_device")

    def contains_device(self, n, nullifier, found, stream=None):
        d = Engine._dp
        self._chk(self._lib.plume_nullset_contains_device(self._handle(), int(n), d(nullifier), d(found), C.c_void_p(self._stream(stream))), "plume_nullset_contains_device")


_default = None


def default_engine() -> Engine:
    global _default
    if _default is None:
        _default = Engine()
    return _default
