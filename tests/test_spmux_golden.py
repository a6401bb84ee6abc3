"""The float64 model of spatial multiplexing and CDD (tests/spmux_model.py) held to what the reference's own functions gave (tests/golden/spmux_ref.npz,
tools/gen_golden_spmux.py).  CPU only: this pins the model the device tests (test_gpu_spmux.py) compare the kernels with, and shows that the chosen inputs keep
the reference itself inside the bounds those tests allow it.

The model is the closed form -- solve(H, y), (H^H H + N0 I)^-1 H^H y, h^H y / |h|^2 with H = channel x precoder -- not a transcription of the reference's
loops.  Bounds: the reference's vector bodies form 1 / |det|^2 (ZF, MMSE) and 1 / |h|^2 (one layer) with a reciprocal estimate (_mm256_rcp_ps: relative error
at most 1.5 x 2^-12), which enters x once and the MMSE csi twice; the scalar tail divides exactly.  So x: per-RE vector error <= 2^-11 |x|; csi: <= 2^-10
relative.  Measured on this fixture: x worst 1.17 x 2^-12 |x| in the vector part and 4.4 x 2^-24 |x| in the scalar tail; csi worst 2.05 x 2^-12."""
import os
import subprocess

import numpy as np
import pytest

import spmux_model as M

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(G, "spmux_ref.npz"))


def test_fixture_covers_every_taken_case(ref):
    assert [tuple(c) for c in ref["cases"]] == M.CASES
    assert [(int(d), float(np.float32(n))) for d, n in ref["decoders"]] == [(d, float(np.float32(n))) for d, n in M.DECODERS]
    assert [float(s) for s in ref["scalings"]] == [float(np.float32(s)) for s in M.SCALINGS]
    assert ref["y"].shape == (2, 516) and ref["h"].shape == (2, 2, 516)  # 512 REs through the 8-wide vector body, 4 through the scalar tail
    assert os.path.getsize(os.path.join(G, "spmux_ref.npz")) < 512 * 1024


def test_model_against_the_reference_record(ref):
    y, h = ref["y"], ref["h"]
    worst_x = worst_tail = worst_csi = 0.0
    for scheme, layers, cb in M.CASES:
        for di, (dec, noise) in enumerate(M.DECODERS):
            if layers == 1 and di > 0:
                continue
            for si, scaling in enumerate(M.SCALINGS):
                tag = "rx_%d_%d_%d_d%d_s%d" % (scheme, layers, cb, di, si)
                x, csi, _ = M.model64(y, h, scheme, layers, cb, dec, noise, scaling)
                rx, rcsi = ref[tag + "_x"], ref[tag + "_csi"]
                err = np.sqrt((np.abs(rx - x) ** 2).sum(0)) / np.sqrt((np.abs(x) ** 2).sum(0))
                worst_x, worst_tail = max(worst_x, float(err.max())), max(worst_tail, float(err[512:].max()))
                assert np.all(err <= 2.0 ** -11), (tag, float(err.max()))
                for k in range(rcsi.shape[0]):
                    if np.isnan(csi[k]).all():  # the row the two-layer ZF multiplex body leaves alone
                        assert np.all(rcsi[k] == ref["csi_sentinel"]), tag
                        continue
                    rel = np.abs(rcsi[k] - csi[k]) / np.abs(csi[k])
                    worst_csi = max(worst_csi, float(rel.max()))
                    assert np.all(rel <= 2.0 ** -10), (tag, k, float(rel.max()))
    print("x: worst %.2f x 2^-12 |x| (scalar tail %.2f x 2^-24); csi: worst %.2f x 2^-12" % (worst_x * 2 ** 12, worst_tail * 2 ** 24, worst_csi * 2 ** 12))


def test_transmit_record_is_the_float32_expression(ref):
    """equal as numbers (-0 equals 0) to (x0 +- x1) * factor evaluated in float32, and within float32 rounding of the float64 model W x"""
    xl = ref["layers"]
    for scheme, layers, cb in M.CASES:
        for si, scaling in enumerate(M.SCALINGS):
            rec = ref["tx_%d_%d_%d_s%d" % (scheme, layers, cb, si)]
            got = M.precode32(xl, scheme, layers, cb, scaling)
            assert np.array_equal(rec, got), (scheme, layers, cb, si, int(np.count_nonzero(rec != got)))
            want = M.precode64(xl, scheme, layers, cb, scaling)
            assert np.all(np.abs(rec - want) <= 4 * M.EPS * (np.abs(xl[:layers]).sum(0) * float(scaling))), (scheme, layers, cb, si)


def test_emulated_operation_order_is_inside_the_bound_of_the_device_tests():
    """the library's fixed operation order, evaluated in float32 on the CPU, against the float64 model on the shapes of test_gpu_spmux.py's first test: the worst
    factor per equaliser is what M.C_BOUND is about five times of"""
    worst = {"zf": 0.0, "mmse": 0.0, "mrc": 0.0}
    rng = np.random.default_rng(2)
    for n in (2, 6, 254, 258, 2046, 2050, 4100, 301):
        y = np.ascontiguousarray(M.cn(rng, (2, n)).astype(np.complex64))
        h = M.channel(rng, n)
        for scheme, layers, cb in M.CASES:
            if scheme == M.TXSCHEME_CDD and n % 2:
                continue
            for dec, noise in M.DECODERS[:1] if layers == 1 else M.DECODERS:
                for scaling in M.SCALINGS:
                    want, wcsi, S = M.model64(y, h, scheme, layers, cb, dec, noise, scaling)
                    x, csi = M.emulate32(y, h, scheme, layers, cb, dec, noise, scaling)
                    k = M.kind_of(layers, dec)
                    worst[k] = max(worst[k], M.worst_factor(x, want, S))
                    keep = ~np.isnan(wcsi)
                    assert np.array_equal(np.isnan(csi), ~keep)
                    assert np.all(np.abs(csi[keep] - wcsi[keep]) <= 64 * M.EPS * np.abs(wcsi[keep])), (n, scheme, layers, cb, dec)
    print("worst factor of the float32 emulation: " + ", ".join("%s %.2f (c = %g)" % (k, v, M.C_BOUND[k]) for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= M.C_BOUND[k] / 4, (k, v)  # c keeps at least a factor 4 of headroom over the emulation


# ---- the header's own source text on the host

_SHIM = """#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define __device__
#define __forceinline__ inline
struct float2 { float x, y; };
struct float4 { float x, y, z, w; };
static inline float2 make_float2(float x, float y) { return float2{x, y}; }
"""
_MAIN = """
// argv: eq layers pre0 pre1 mmse norm noise n | pre kind0 kind1 scale n;  planes of n complex floats on stdin, results on stdout
int main(int argc, char** argv)
{
  const bool eq = argv[1][0] == 'e';
  const size_t n = atol(argv[eq ? 8 : 5]);
  std::vector<float2> pl[6], x0(n), x1(n);
  std::vector<float> c0(n), c1(n);
  for (int k = 0; k < (eq ? 6 : 2); k++) { pl[k].resize(n); if (fread(pl[k].data(), 8, n, stdin) != n) return 1; }
  for (size_t i = 0; i < n; i++) {
    x1[i] = make_float2(0, 0); c0[i] = c1[i] = 0;
    if (eq) {
      const uint32_t pre[2] = {(uint32_t)atoi(argv[3]), (uint32_t)atoi(argv[4])};
      mimo_equalise(atoi(argv[2]), pre[i & 1], atoi(argv[5]) != 0, pl[0][i], pl[1][i], pl[2][i], pl[3][i], pl[4][i], pl[5][i], strtof(argv[6], nullptr), strtof(argv[7], nullptr),
                    x0[i], x1[i], c0[i], c1[i]);
    } else {
      const uint32_t kind[2] = {(uint32_t)atoi(argv[2]), (uint32_t)atoi(argv[3])};
      mimo_precode(kind[i & 1], pl[0][i], pl[1][i], strtof(argv[4], nullptr), x0[i], x1[i]);
    }
  }
  fwrite(x0.data(), 8, n, stdout); fwrite(x1.data(), 8, n, stdout); fwrite(c0.data(), 4, n, stdout); fwrite(c1.data(), 4, n, stdout);
  return 0;
}
"""


@pytest.fixture(scope="module")
def host_arith():
    """the 2x2 section of csrc/modem_arith.h and the enums it uses from modem_device.h, cut out of the files as they are, compiled for the host with the device
    qualifiers defined away and without contraction: what the kernels' source says, evaluated in IEEE float32"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "srslte_amd", "csrc", "modem_arith.h")).read()
    body = src[src.index("// ---- 2x2 spatial multiplexing and large-delay CDD"):src.index("// ---- scrambling chips of one tile")]
    dev = open(os.path.join(root, "srslte_amd", "csrc", "modem_device.h")).read()
    enums = dev[dev.index("enum { PRE_PLUS"):dev.index("struct Job")]
    assert "__fmul_rn(" not in body and "__fadd_rn(" not in body and "__fsub_rn(" not in body and body.count("#pragma clang fp contract(off)") == 4  # every operation goes through rn_*
    d = os.path.join(root, "build", "scratch")
    os.makedirs(d, exist_ok=True)
    cfile, exe = os.path.join(d, "spmux_arith_host.cpp"), os.path.join(d, "spmux_arith_host")
    open(cfile, "w").write(_SHIM + enums + body + _MAIN)
    subprocess.check_call(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-Wno-unknown-pragmas", "-o", exe, cfile])
    return exe


def _pre_of(scheme, layers, cb):
    return (cb, cb) if layers == 1 or scheme == M.TXSCHEME_SPATIALMUX else (1, 3)  # HEFF_PM / HEFF_MP on the even / odd REs of CDD


def test_header_equalisers_on_the_host_are_the_emulation(host_arith):
    """mimo_equalise as csrc/modem_arith.h states it, bit for bit what spmux_model.emulate32 gives: the emulation the bound's constant comes from is the
    kernels' operation order, not a transcription that could drift from it"""
    rng = np.random.default_rng(5)
    for scheme, layers, cb in M.CASES:
        n = 516 if scheme == M.TXSCHEME_CDD else 517
        y, h = np.ascontiguousarray(M.cn(rng, (2, n)).astype(np.complex64)), M.channel(rng, n)
        for dec, noise in (M.DECODERS[:1] if layers == 1 else M.DECODERS):
            for scaling in M.SCALINGS:
                two = layers == 2 and (scheme == M.TXSCHEME_CDD or cb > 0)
                norm = (np.float32(2.0) if two else np.float32(np.sqrt(2.0))) / np.float32(scaling)
                pre = _pre_of(scheme, layers, cb)
                out = subprocess.run([host_arith, "eq", str(layers), str(pre[0]), str(pre[1]), str(int(dec == M.MMSE)), repr(float(norm)), repr(float(np.float32(noise))), str(n)],
                                     input=b"".join(a.tobytes() for a in (y[0], y[1], h[0][0], h[1][0], h[0][1], h[1][1])), capture_output=True, check=True).stdout
                x = np.frombuffer(out[:16 * n], np.complex64).reshape(2, n)
                c = np.frombuffer(out[16 * n:], np.float32).reshape(2, n)
                ex, ec = M.emulate32(y, h, scheme, layers, cb, dec, noise, scaling)
                for k in range(layers):
                    assert np.array_equal(x[k].view(np.uint32), ex[k].view(np.uint32)), (scheme, layers, cb, dec, noise, scaling, k)
                    if not np.isnan(ec[k]).all():
                        assert np.array_equal(c[k].view(np.uint32), ec[k].view(np.uint32)), (scheme, layers, cb, dec, noise, scaling, k)


def test_header_precoder_on_the_host_is_the_reference_record(host_arith, ref):
    """mimo_precode as csrc/modem_arith.h states it, with the factor the host code forms, equal as numbers to what the reference's functions gave"""
    xl = np.ascontiguousarray(ref["layers"])
    n = xl.shape[1]
    for scheme, layers, cb in M.CASES:
        for si, scaling in enumerate(M.SCALINGS):
            s = np.float32(scaling)
            if scheme == M.TXSCHEME_CDD:
                kind, f = (0, 1), s / np.float32(2)  # TXPRE_CDD + parity
            elif layers == 2:
                kind, f = (2 + cb, 2 + cb), (np.float32(np.float64(s) * np.sqrt(0.5)) if cb == 0 else s / np.float32(2))  # TXPRE_MUX2 + codebook_idx
            else:
                kind, f = (5 + cb, 5 + cb), np.float32(np.float64(s) * np.sqrt(0.5))  # TXPRE_MUX1 + codebook_idx
            out = subprocess.run([host_arith, "pre", str(kind[0]), str(kind[1]), repr(float(f)), str(n)], input=xl[0].tobytes() + xl[1].tobytes(), capture_output=True, check=True).stdout
            got = np.frombuffer(out[:16 * n], np.complex64).reshape(2, n)
            want = ref["tx_%d_%d_%d_s%d" % (scheme, layers, cb, si)]
            assert np.array_equal(got, want), (scheme, layers, cb, si, int(np.count_nonzero(got != want)))
