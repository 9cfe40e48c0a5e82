"""TEST INFRASTRUCTURE, NOT PRODUCT CODE: pysdm_amd/csrc/pair_tag.h on the host.

`model()` compiles tests/pair_tag_model/pair_tag_model.c - loops over the header's own functions -
with the compiler and flags of the oracle into a temporary directory, once per process, and
returns numpy-shaped wrappers.  tests/test_pair_tag_model.py and scripts/pair_tag_share.py use it;
nothing under pysdm_amd/ imports this package.
"""
import atexit
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "pair_tag_model.c")
_FLAGS = ["-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
          "-fvisibility=hidden"]  # oracle/engine.py

I64, F64, U32 = ctypes.c_int64, ctypes.c_double, ctypes.c_uint32


def _ptr(array, ctype):
    return array.ctypes.data_as(ctypes.POINTER(ctype))


class Model:
    def __init__(self, lib):
        self.lib = lib
        lib.pt_m_base.restype = F64
        lib.pt_m_base.argtypes = [F64]
        self.shift, self.bits = lib.pt_shift(), lib.pt_bits()

    def m_base(self, m_max):
        return float(self.lib.pt_m_base(float(m_max)))

    def encode(self, n, m, n_ref, m_base):
        n = np.ascontiguousarray(n, dtype=np.int64)
        m = np.ascontiguousarray(m, dtype=np.float64)
        tag = np.zeros(n.shape, dtype=np.uint32)
        self.lib.pt_encode(_ptr(n, I64), _ptr(m, F64), I64(n.size), I64(int(n_ref)),
                           F64(m_base), _ptr(tag, U32))
        return tag

    def bounds(self, tag, n_ref, m_base):
        tag = np.ascontiguousarray(tag, dtype=np.uint32)
        n_ub = np.zeros(tag.shape, dtype=np.int64)
        m_ub = np.zeros(tag.shape, dtype=np.float64)
        self.lib.pt_bounds(_ptr(tag, U32), I64(tag.size), I64(int(n_ref)), F64(m_base),
                           _ptr(n_ub, I64), _ptr(m_ub, F64))
        return n_ub, m_ub

    def order(self, tag_j, tag_k):
        tag_j = np.ascontiguousarray(tag_j, dtype=np.uint32)
        tag_k = np.ascontiguousarray(tag_k, dtype=np.uint32)
        out = np.zeros(tag_j.shape, dtype=np.int8)
        self.lib.pt_order(_ptr(tag_j, U32), _ptr(tag_k, U32), I64(tag_j.size),
                          out.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)))
        return out

    def decide(self, tag_j, tag_k, u, *, n_ref, m_base, b, rho_w, norm, substeps=1):
        """(skipped, swap) per pair"""
        tag_j = np.ascontiguousarray(tag_j, dtype=np.uint32)
        tag_k = np.ascontiguousarray(tag_k, dtype=np.uint32)
        u = np.ascontiguousarray(u, dtype=np.float64)
        skipped = np.zeros(tag_j.shape, dtype=np.uint8)
        swap = np.zeros(tag_j.shape, dtype=np.uint8)
        self.lib.pt_decide(_ptr(tag_j, U32), _ptr(tag_k, U32), _ptr(u, F64), I64(tag_j.size),
                           I64(int(n_ref)), F64(m_base), F64(b), F64(rho_w), F64(norm),
                           I64(int(substeps)), _ptr(skipped, ctypes.c_uint8),
                           _ptr(swap, ctypes.c_uint8))
        return skipped.astype(bool), swap.astype(bool)


@functools.lru_cache(maxsize=None)
def model():
    directory = tempfile.mkdtemp(prefix="pair_tag_model_")
    atexit.register(shutil.rmtree, directory, ignore_errors=True)
    path = os.path.join(directory, "libpair_tag_model.so")
    subprocess.check_call(["gcc", *_FLAGS, "-o", path, SOURCE])
    return Model(ctypes.CDLL(path))


def norm_factor(dt, dv, n_live):
    """collisions_methods.py:643-650, left to right, for the one cell of a box"""
    if n_live < 2:
        return 0.0
    return dt / dv * float(n_live) * float(n_live - 1) / 2 / float(n_live // 2)


def full_prob(multiplicity, mass, j, k, *, b, rho_w, norm, substeps=1):
    """the probability of the pairs (j, k) as the oracle computes it, array operation by array
    operation in float64 (oracle/sdm_oracle_abi.c, box_step: box_kernel's Golovin case on
    box_volume, the pair maximum of the multiplicities, times the kernel, oracle_normalize,
    divided by the sub-steps) - nothing of pair_tag.h or of its model in C"""
    volume = np.asarray(mass, dtype=np.float64) / rho_w
    kernel = (volume[j] + volume[k]) * b
    prob = np.maximum(multiplicity[j], multiplicity[k]).astype(np.float64)
    prob = prob * kernel
    prob = prob * norm
    return prob / float(substeps)


def skip_share(mdl, multiplicity, mass, ids, rng, *, n_ref, m_base, b, rho_w, dt, dv, substeps=1):
    """one random pairing of the live ids: (pairs, skipped, colliding, sound) - `sound`: every
    skipped pair has gamma == 0 and the decided order in the full computation"""
    ids = np.asarray(ids, dtype=np.int64)
    shuffled = ids[rng.permutation(len(ids))]
    pairs = len(shuffled) // 2
    j, k = shuffled[0:2 * pairs:2], shuffled[1:2 * pairs:2]
    u = rng.random(pairs)
    tags = mdl.encode(multiplicity, mass, n_ref, m_base)
    norm = norm_factor(dt, dv, len(ids))
    skipped, swap = mdl.decide(tags[j], tags[k], u, n_ref=n_ref, m_base=m_base, b=b, rho_w=rho_w,
                               norm=norm, substeps=substeps)
    full_swap = multiplicity[j] < multiplicity[k]
    prob = full_prob(multiplicity, mass, j, k, b=b, rho_w=rho_w, norm=norm, substeps=substeps)
    gamma = np.ceil(prob - u)
    sound = bool(np.all(gamma[skipped] == 0) and np.all(swap[skipped] == full_swap[skipped]))
    return pairs, int(skipped.sum()), int((gamma != 0).sum()), sound
