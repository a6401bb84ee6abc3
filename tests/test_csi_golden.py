"""The numpy model of the CSI weighting (tests/csi_model.py) held to what the reference's own csi_correction gave (tests/golden/csi_ref.npz,
tools/gen_golden_csi.py): every soft bit of every case, equal.  CPU only: this pins the model the device tests (test_gpu_pdsch_csi.py) hold the kernel to.
The second half compiles the kernel's per-bit function, cut out of csrc/csi_kernels.hip as it is, for the host and holds it to the same record."""
import os
import subprocess

import numpy as np
import pytest

import csi_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "csi_ref.npz")


@pytest.fixture(scope="module")
def ref():
    return np.load(FIXTURE)


def test_fixture_covers_every_modulation_width_and_size(ref):
    assert os.path.getsize(FIXTURE) < 256 * 1024
    cases = {(int(m), int(w), int(n), str(k)) for (m, w, n), k in zip(ref["cases"], ref["kinds"])}
    for mod in range(5):
        for llr8 in (0, 1):
            for n in (2, 3, 8, 301, 516):
                assert (mod, llr8, n, "rand") in cases
            for kind in ("equal", "ratio", "tiny"):
                assert any(c[0] == mod and c[1] == llr8 and c[3] == kind for c in cases)
    for i, ((mod, llr8, n), kind) in enumerate(zip(ref["cases"], ref["kinds"])):
        e, c = ref["e_%d" % i], ref["csi_%d" % i]
        assert e.dtype == (np.int8 if llr8 else np.int16) and e.size == n * M.QM[int(mod)] and c.dtype == np.float32 and c.size == n and np.all(c > 0)
        info = np.iinfo(e.dtype)
        assert set([0, 1, -1, info.max, info.min][:e.size]) <= set(e.tolist())  # 0, +-1 and the extremes are among the soft bits
        if kind == "equal":
            assert np.all(c == c[0])
        if kind == "ratio":
            assert 0.99e4 < c.max() / c.min() < 1.01e4
    # the position of the maximum differs between the random cases
    assert len({int(np.argmax(ref["csi_%d" % i])) for i in range(len(ref["cases"])) if ref["cases"][i][2] == 516}) > 3


def test_model_equals_the_reference_record(ref):
    for i, (mod, llr8, n) in enumerate(ref["cases"]):
        got = M.csi_model(ref["e_%d" % i], ref["csi_%d" % i], int(mod), bool(llr8))
        want = ref["out_%d" % i]
        assert got.dtype == want.dtype and np.array_equal(got, want), (int(mod), int(llr8), int(n), str(ref["kinds"][i]), int(np.count_nonzero(got != want)))


def test_record_shows_the_quirks_the_model_carries(ref):
    """what makes the weighting more than e * c / c_max: the halved 16-bit body, the untouched-in-scale left-over symbol, the pair swap"""
    e = np.full(10, 1000, np.int16)
    out = M.csi_model(e, np.arange(1, 6, dtype=np.float32), 1, False)
    assert out.tolist() == [199, 199, 99, 99, 399, 399, 299, 299, 1000, 1000]  # QPSK: each pair takes the other's weight; the fifth symbol is left over
    assert M.csi_model(np.array([-1, -3, 1, 3], np.int16), np.ones(1, np.float32), 2, False).tolist() == [-1, -2, 0, 1]  # w = 32767, >> 16 floors
    t, vec = M.weight_symbol(3, 3)
    assert t[:2].reshape(-1).tolist() == [0, 0, 0, 0, 1, 1, 0, 0, 1, 1, 1, 1] and vec.tolist() == [True, True, False]


# ---- the kernel's own source text on the host

_SHIM = """#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define __device__
#define __forceinline__ inline
using std::min;
using std::max;
static inline int __float2int_rn(float x) { return (int)std::nearbyintf(x); }  // round to nearest even (the default rounding mode)
"""
_MAIN = """
// argv: mod llr8 n; csi (n floats) then the soft bits on stdin, the weighted soft bits on stdout
template <typename T>
int run(int mod, uint32_t n)
{
  const uint32_t qm = mod == 0 ? 1 : 2 * mod;
  std::vector<float> c(n);
  std::vector<T> e((size_t)n * qm);
  if (fread(c.data(), 4, n, stdin) != n || fread(e.data(), sizeof(T), e.size(), stdin) != e.size()) return 1;
  const float c_max = *std::max_element(c.begin(), c.end()), scale = rn_div(32767.0f, c_max);
  for (uint32_t b = 0; b < e.size(); b++) {
    switch (mod) {
      case 0: e[b] = weigh<T, 0>(e[b], b, c.data(), n, c_max, scale); break;
      case 1: e[b] = weigh<T, 1>(e[b], b, c.data(), n, c_max, scale); break;
      case 2: e[b] = weigh<T, 2>(e[b], b, c.data(), n, c_max, scale); break;
      case 3: e[b] = weigh<T, 3>(e[b], b, c.data(), n, c_max, scale); break;
      default: e[b] = weigh<T, 4>(e[b], b, c.data(), n, c_max, scale); break;
    }
  }
  fwrite(e.data(), sizeof(T), e.size(), stdout);
  return 0;
}
int main(int argc, char** argv)
{
  return atoi(argv[2]) ? run<int8_t>(atoi(argv[1]), atol(argv[3])) : run<int16_t>(atoi(argv[1]), atol(argv[3]));
}
"""


@pytest.fixture(scope="module")
def host_weigh():
    """`weigh` of csrc/csi_kernels.hip and rn_mul / rn_div of csrc/modem_arith.h, cut out of the files as they are and compiled for the host without
    contraction: what the kernel's source says per soft bit, evaluated in IEEE float32"""
    csrc = os.path.join(ROOT, "srslte_amd", "csrc")
    arith = open(os.path.join(csrc, "modem_arith.h")).read()
    rn = arith[arith.index("__device__ __forceinline__ float rn_mul(float a, float b)\n{"):arith.index("__device__ __forceinline__ float2 lo(")]
    src = open(os.path.join(csrc, "csi_kernels.hip")).read()
    body = src[src.index("// soft bit `b` of the codeword"):src.index("template <typename T, int MOD>\n__device__ __forceinline__ void weigh_tile")]
    d = os.path.join(ROOT, "build", "scratch")
    os.makedirs(d, exist_ok=True)
    cfile, exe = os.path.join(d, "csi_weigh_host.cpp"), os.path.join(d, "csi_weigh_host")
    open(cfile, "w").write(_SHIM + rn + body + _MAIN)
    subprocess.check_call(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-Wno-unknown-pragmas", "-o", exe, cfile])
    return exe


def test_kernel_source_on_the_host_equals_the_reference_record(host_weigh, ref):
    for i, (mod, llr8, n) in enumerate(ref["cases"]):
        out = subprocess.run([host_weigh, str(int(mod)), str(int(llr8)), str(int(n))], input=ref["csi_%d" % i].tobytes() + ref["e_%d" % i].tobytes(), capture_output=True,
                             check=True).stdout
        want = ref["out_%d" % i]
        got = np.frombuffer(out, want.dtype)
        assert np.array_equal(got, want), (int(mod), int(llr8), int(n), str(ref["kinds"][i]), int(np.count_nonzero(got != want)))
