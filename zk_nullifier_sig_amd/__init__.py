"""Import alias: the package directory is named `zk-nullifier-sig_amd/` (not a valid Python identifier), so this
shim package extends its search path to that directory and re-exports it.  `import zk_nullifier_sig_amd as plume`."""
from pathlib import Path as _Path

__path__.append(str(_Path(__file__).resolve().parent.parent / "zk-nullifier-sig_amd"))

from .capi import ECDSA_INVALID, ECDSA_LOW_S, ECDSA_MATCH, ECDSA_MISMATCH, ECDSA_SIGN_V27, ETH_HASH_MODES, ETH_INVALID, ETH_MATCH, ETH_MISMATCH, ETH_TX_INVALID, ETH_TX_OK, ETH_TX_SIGN_GROWTH, HD_HARDENED, HD_MAX_DEPTH, HD_SHARED_PARENT, HD_SHARED_PATH, KDF_BIP39, KDF_MAX_ITERATIONS, KDF_MAX_SALT, KDF_SHARED_SALT, MERKLE_BAD_PROOF, MERKLE_INVALID, MERKLE_MATCH, MERKLE_MISMATCH, Engine, MerkleTree, NullifierSet, PlumeHipError, STATUS_BAD_TX, STATUS_HD_HARDENED, STATUS_HD_NO_KEY, STATUS_KDF_BAD_INPUT, bip39_bytes, default_engine, library_path  # noqa: E402,F401
from .plume import (  # noqa: E402,F401
    DST,
    AffinePoint,
    NonZeroScalar,
    PlumePanic,
    PlumeSelfCheckError,
    PlumeSignature,
    PlumeSignaturePrivate,
    PlumeSignaturePublic,
    PlumeSignatureV1Fields,
    PlumeSigner,
    PlumeVersion,
    SecretKey,
    SignatureError,
    circuit_inputs,
    circuit_outputs,
    ecdsa_recover,
    ecdsa_recover_address,
    ecdsa_sign,
    merkle_leaf,
    merkle_proof,
    merkle_root,
    merkle_verify,
    personal_recover,
    personal_sign,
    sign,
    sign_with_r,
    sign_tx,
    hd_address,
    hd_derive,
    hd_derive_pub,
    hd_master,
    mnemonic_to_address,
    mnemonic_to_seed,
    pbkdf2_sha512,
    parse_path,
    parse_xprv,
    parse_xpub,
    tx_sender,
    tx_sender_address,
    tx_signing_hash,
    verify_non_zk,
)
from . import nullifier_set  # noqa: E402,F401
