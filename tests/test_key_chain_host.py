"""The key chain the host derives for the first links of a run (d3p_key_chain_host; d3p_dpvi.hip: host_key_chain) against the
oracle's split, link by link: k_{t+1} = split(k_t, 3)[0], and each link's three children.  No GPU involved."""
import ctypes as C

import numpy as np

from oracle import oracle as O


def _host_chain(key, n):
    import d3p_amd._lib as L
    L.build()
    lib = L.load()
    out = np.zeros((n, 3, 16), np.uint32)
    k = np.ascontiguousarray(np.asarray(key, np.uint32).reshape(16))
    L.check(lib.d3p_key_chain_host(k.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p)))
    return out


def test_host_key_chain_matches_oracle_split_over_150_links():
    for seed in (0, 3, 0x7FFFFFFF):
        key = np.asarray(O.PRNGKey(seed), np.uint32).reshape(16)
        got = _host_chain(key, 150)
        cur = key
        for t in range(150):
            want = np.asarray(O.split(cur, 3), np.uint32).reshape(3, 16)
            assert np.array_equal(got[t], want), (seed, t)
            cur = want[0]


def test_host_key_chain_from_a_key_with_nonzero_counter_words():
    # (a key given by the caller need not be a derived one: its counter / nonce words are taken as they are)
    key = np.arange(1, 17, dtype=np.uint32) * np.uint32(0x9E3779B9)
    got = _host_chain(key, 3)
    cur = key
    for t in range(3):
        want = np.asarray(O.split(cur, 3), np.uint32).reshape(3, 16)
        assert np.array_equal(got[t], want), t
        cur = want[0]
    assert _host_chain(key, 0).shape == (0, 3, 16)
