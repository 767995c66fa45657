"""Builds the reference's own hot path into oracle/_ref/ and runs it.

TEST INFRASTRUCTURE ONLY.  Three executables are compiled from the reference's translation units, UNCHANGED, against the
stand-in headers of oracle/ref_shim/ (the i2l library is not vendored with the reference) and the project's own drivers:

    ref_score_dna, ref_score_aa   ipk/src/window.cpp + ipk/src/pk_compute.cpp + oracle/ref_driver_score.cpp
    ref_mif0                      ipk/src/filter.cpp + oracle/ref_driver_mif0.cpp

The reference tree is looked up in $IPK_REFERENCE_DIR (default /root/reference).  Where it does not exist nothing is built and
nothing is removed: binaries built elsewhere and carried along keep working (they are linked with a static libstdc++ for that).
No reference file and nothing compiled from one is ever committed: oracle/_ref/ is ignored by git.
"""
import os
import struct
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
SHIM_DIR = os.path.join(_HERE, "ref_shim")

CXX = os.environ.get("CXX", "g++")
# one rounding per operation, as the oracle (oracle/Makefile): no contraction, no fast-math, no -march=native
CXXFLAGS = ["-std=c++17", "-O2", "-ffp-contract=off"]
LDFLAGS = ["-static-libstdc++", "-static-libgcc"]

# name: (reference sources, driver, extra flags)
TARGETS = {
    "ref_score_dna": (("ipk/src/window.cpp", "ipk/src/pk_compute.cpp"), "ref_driver_score.cpp", ()),
    "ref_score_aa": (("ipk/src/window.cpp", "ipk/src/pk_compute.cpp"), "ref_driver_score.cpp", ("-DSEQ_TYPE_AA",)),
    "ref_mif0": (("ipk/src/filter.cpp",), "ref_driver_mif0.cpp", ()),
}


def reference_dir():
    return os.environ.get("IPK_REFERENCE_DIR", "/root/reference")


def binary(name):
    return os.path.join(REF_DIR, name)


def present():
    """The names of the binaries that exist in oracle/_ref/."""
    return [n for n in TARGETS if os.path.isfile(binary(n)) and os.access(binary(n), os.X_OK)]


def available():
    """True when all three reference binaries are there to be run."""
    return len(present()) == len(TARGETS)


def _shim_files():
    out = []
    for d, _, files in os.walk(SHIM_DIR):
        out += [os.path.join(d, f) for f in files]
    return out


def build(force=False, verbose=False):
    """Compile the three executables into oracle/_ref/ (only those missing or older than one of their inputs, unless `force`).
    Returns the names of the binaries present afterwards.  Without the reference tree: leaves oracle/_ref/ as found."""
    ref = reference_dir()
    if not os.path.isdir(os.path.join(ref, "ipk", "src")):
        if verbose:
            print(f"oracle/_ref: no reference tree at {ref}; present: {present() or 'nothing'}")
        return present()
    os.makedirs(REF_DIR, exist_ok=True)
    for name, (sources, driver, extra) in TARGETS.items():
        inputs = [os.path.join(ref, s) for s in sources] + [os.path.join(_HERE, driver)] + _shim_files()
        out = binary(name)
        if not force and os.path.isfile(out) and all(os.path.getmtime(out) >= os.path.getmtime(i) for i in inputs):
            continue
        cmd = [CXX] + CXXFLAGS + list(extra) + ["-I", os.path.join(ref, "ipk", "include"), "-I", SHIM_DIR]
        cmd += [os.path.join(ref, s) for s in sources] + [os.path.join(_HERE, driver), "-o", out + ".tmp"] + LDFLAGS
        if verbose:
            print("oracle/_ref:", " ".join(cmd))
        subprocess.check_call(cmd)
        os.replace(out + ".tmp", out)
    return present()


# ---- running them ------------------------------------------------------------------------------------------------------------------

def _eps_bits(eps):
    return int(np.array([eps], dtype=np.float32).view(np.uint32)[0])


def _score_binary(sigma):
    if sigma not in (4, 20):
        raise ValueError("sigma must be 4 or 20")
    return binary("ref_score_dna" if sigma == 4 else "ref_score_aa")


def ref_windows_many(mats, k, eps, sigma):
    """The reference's DCLA over every window of every matrix of mats [n_mats, sites, sigma], in ONE process.
    Returns, per matrix, the list of (position, keys uint32, score bits uint32) in to_windows order; the k-mers of a window
    are in the reference's emission order."""
    mats = np.ascontiguousarray(mats, dtype=np.float32)
    n_mats, sites, s = mats.shape
    if s != sigma or sites < k or k < 1:
        raise ValueError("need [n_mats, sites >= k, sigma] matrices")
    inp = struct.pack("=4I", n_mats, sites, k, _eps_bits(eps)) + mats.tobytes()
    out = subprocess.run([_score_binary(sigma)], input=inp, stdout=subprocess.PIPE, check=True).stdout
    res, at = [], 0
    for _ in range(n_mats):
        wins = []
        for _ in range(sites - k + 1):
            pos, cnt = struct.unpack_from("=2Q", out, at)
            at += 16
            pairs = np.frombuffer(out, dtype=np.uint32, count=2 * cnt, offset=at).reshape(cnt, 2)
            at += 8 * cnt
            wins.append((int(pos), pairs[:, 0].copy(), pairs[:, 1].copy()))
        res.append(wins)
    if at != len(out):
        raise RuntimeError("reference binary wrote more windows than to_windows should give")
    return res


def ref_windows(m, k, eps, sigma):
    """One matrix m [sites, sigma]: [(window.get_position(), keys uint32, score bits uint32), ...] as the reference emits them."""
    return ref_windows_many(np.asarray(m, dtype=np.float32)[None], k, eps, sigma)[0]


def merge_windows(per_matrix, positions=False):
    """The group's max-merge over per-window lists (matrices in order, windows in order, k-mers in emission order)."""
    keys = [w[1] for wins in per_matrix for w in wins]
    bits = [w[2] for wins in per_matrix for w in wins]
    pos = [np.full(len(w[1]), w[0], dtype=np.uint32) for wins in per_matrix for w in wins]
    keys = np.concatenate(keys) if keys else np.zeros(0, np.uint32)
    scores = (np.concatenate(bits) if bits else np.zeros(0, np.uint32)).view(np.float32)
    pos = np.concatenate(pos) if pos else np.zeros(0, np.uint32)
    emitted = len(keys)
    # per key: the largest score, and of the entries that reach it the first to arrive (a stored score is replaced only when it
    # is strictly smaller).  lexsort is stable: by key, then by descending score, then by arrival.
    with np.errstate(invalid="ignore"):
        order = np.lexsort((-scores, keys))
    keys, scores, pos = keys[order], scores[order], pos[order]
    first = np.ones(emitted, dtype=bool)
    first[1:] = keys[1:] != keys[:-1]
    if positions:
        return keys[first], scores[first], pos[first], emitted
    return keys[first], scores[first], emitted


def ref_explore_group(mats, k, eps, sigma, positions=False):
    """explore_group of one branch group from the reference's per-window output: (keys ascending, scores float32, emitted), or
    with positions=True (keys, scores, positions of the first window reaching the kept score, emitted).

    The per-window lists come from the compiled reference (ref_windows_many).  The merge across windows and matrices does NOT:
    it is a restatement of ipk::put (ipk/src/branch_group.cpp:73-100) -- a stored score is replaced only when it is strictly
    smaller (`<`), so the first window of the first matrix wins a tie -- because branch_group.cpp needs boost serialisation and
    is not compiled."""
    return merge_windows(ref_windows_many(mats, k, eps, sigma), positions)


def ref_mif0(lists, N, thr):
    """mif0_filter::calc_filter_values of the compiled reference: one double per entry list (log10 scores, in entry order), for
    a database of N groups and the float threshold thr."""
    lists = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in lists]
    if not lists:
        return np.zeros(0, np.float64)
    inp = [struct.pack("=Q2I", int(N), _eps_bits(thr), len(lists))]
    for a in lists:
        if a.size == 0 or a.size > N:
            raise ValueError("an entry list needs 1..N entries")
        inp.append(struct.pack("=I", a.size) + a.tobytes())
    out = subprocess.run([binary("ref_mif0")], input=b"".join(inp), stdout=subprocess.PIPE, check=True).stdout
    fv = np.frombuffer(out, dtype=np.float64)
    if len(fv) != len(lists):
        raise RuntimeError("reference binary returned the wrong number of filter values")
    return fv.copy()


if __name__ == "__main__":
    print("oracle/_ref:", build(verbose=True))
