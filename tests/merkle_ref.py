"""Checker for the RFC-6962 trees: tendermint crypto/merkle HashFromByteSlices restated with
hashlib. Test code only: the product computes every hash on the device."""
import hashlib


def _sha(b):
    return hashlib.sha256(b).digest()


def hash_from_byte_slices(items):
    """merkle.HashFromByteSlices: SHA256("") for no items, SHA256(0x00 || item) for one,
    else SHA256(0x01 || left || right) split at the largest power of two below the count."""
    if not items:
        return _sha(b"")
    if len(items) == 1:
        return _sha(b"\x00" + items[0])
    k = 1
    while k * 2 < len(items):
        k *= 2
    return _sha(b"\x01" + hash_from_byte_slices(items[:k]) + hash_from_byte_slices(items[k:]))
