"""Expected words for the sponge calls, restated from the reference text on top of the oracle's Tip5 permutation and absorb (both
pinned by the reference's known-answer vectors, tests/test_oracle_kat.py):
  Tip5::new(Domain)            tip5/mod.rs:511-526
  Sponge::absorb / squeeze     tip5/mod.rs:684-698
  Sponge::pad_and_absorb_all   util_types/sponge.rs:41-55
  Tip5::sample_indices         tip5/mod.rs:636-656
  Tip5::sample_scalars         tip5/mod.rs:664-674
A state is 16 raw Montgomery words (numpy uint64); every function returns the new state next to what it produces.  The reference
has no known-answer vectors for the samplers; tests/test_sponge_cpu.py checks this restatement against facts that do not depend
on it."""
import numpy as np

from oracle import tfo

P = (1 << 64) - (1 << 32) + 1
RATE = 10
ONE_RAW = 0xFFFFFFFF                      # BFieldElement::ONE as a raw word (2^64 mod p)
R_INV = pow((1 << 64) % P, P - 2, P)
MAX_RAW = (P - 1) * ((1 << 64) % P) % P   # BFieldElement::new(BFieldElement::MAX) as a raw word
assert MAX_RAW == 0xFFFFFFFE00000002


def value(raw: int) -> int:
    """BFieldElement::value(): the canonical value of a raw word."""
    return int(raw) % P * R_INV % P


def init(fixed_length: bool = False) -> np.ndarray:
    s = np.zeros(16, dtype=np.uint64)
    if fixed_length:
        s[RATE:] = ONE_RAW
    return s


def absorb(state, chunk) -> np.ndarray:
    return tfo.absorb(state, np.asarray(chunk, dtype=np.uint64))


def absorb_many(state, chunks) -> np.ndarray:
    s = np.asarray(state, dtype=np.uint64).copy()
    for c in np.asarray(chunks, dtype=np.uint64).reshape(-1, RATE):
        s = absorb(s, c)
    return s


def squeeze(state):
    s = np.asarray(state, dtype=np.uint64)
    return tfo.tip5_permutation(s), s[:RATE].copy()


def squeeze_many(state, k: int):
    s, out = np.asarray(state, dtype=np.uint64).copy(), np.zeros((k, RATE), dtype=np.uint64)
    for i in range(k):
        s, out[i] = squeeze(s)
    return s, out


def pad_and_absorb_all(state, words) -> np.ndarray:
    w = np.asarray(words, dtype=np.uint64).reshape(-1)
    s = np.asarray(state, dtype=np.uint64).copy()
    full = w.size // RATE
    for c in range(full):
        s = absorb(s, w[c * RATE:(c + 1) * RATE])
    last = np.zeros(RATE, dtype=np.uint64)
    rem = w.size - full * RATE
    last[:rem] = w[full * RATE:]
    last[rem] = ONE_RAW
    return absorb(s, last)


def sample_scalars(state, num_elements: int):
    num_squeezes = -(-(num_elements * 3) // RATE)
    s, out = squeeze_many(state, num_squeezes)
    return s, out.reshape(-1)[:3 * num_elements].reshape(num_elements, 3).copy()


def sample_indices(state, upper_bound: int, num_indices: int):
    assert upper_bound > 0 and upper_bound & (upper_bound - 1) == 0, "upper_bound.is_power_of_two()"
    s = np.asarray(state, dtype=np.uint64).copy()
    indices, buffer, next_in_buffer = [], None, RATE
    while len(indices) < num_indices:
        if next_in_buffer == RATE:
            s, buffer = squeeze(s)
            next_in_buffer = 0
        element = value(buffer[next_in_buffer])
        next_in_buffer += 1
        if element != P - 1:
            indices.append((element & 0xFFFFFFFF) % upper_bound)
    return s, np.array(indices, dtype=np.uint32)
