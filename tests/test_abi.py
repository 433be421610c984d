"""The C-ABI library loads and exports every symbol include/*.h declares (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import ksim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = [os.path.join(ROOT, "include", h) for h in ("ksim_engine.h", "ksim_trace.h")]


def declared_functions():
    names = set()
    for h in HEADERS:
        src = open(h).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        for m in re.finditer(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\**\s*(ksim_[a-z_0-9]+)\s*\(", src, flags=re.M):
            names.add(m.group(1))
    return names


def test_library_exports_every_declared_symbol():
    names = declared_functions()
    assert len(names) >= 25
    L = ksim.lib()
    for n in sorted(names):
        assert hasattr(L, n), n
    out = subprocess.run(["nm", "-D", "--defined-only", ksim.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (ksim_[a-z_0-9]+)", out))
    assert names <= exported
    # the Python binding covers exactly the declared surface
    assert set(ksim.SIGNATURES) == names


def test_struct_layouts_match_c(tmp_path):
    src = os.path.join(ROOT, "tests", "golden", "abi_sizes.c")
    exe = str(tmp_path / "ksim_abi_sizes")
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    got = list(map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()))
    want = [C.sizeof(t) for t in (ksim.Node, ksim.Pod, ksim.Typical, ksim.Result, ksim.Config, ksim.TraceNode,
                                  ksim.TracePod, ksim.TypicalCfg, ksim.ReplayCfg, ksim.Report, ksim.PowerReport,
                                  ksim.PowerModel)]
    assert got == want


def test_abi_version_and_errors():
    L = ksim.lib()
    assert L.ksim_abi_version() == 2
    msgs = [L.ksim_strerror(code) for code in range(0, -10, -1)]
    assert all(msgs) and len(set(msgs)) == len(msgs) and L.ksim_strerror(-10) == b"unknown error"
    # null / bad arguments are rejected before any device work
    assert L.ksim_engine_create(None, 0, 1, None) == ksim.KSIM_EINVAL


def test_no_cpu_fallback_without_device():
    if ksim.device_count() > 0:
        pytest.skip("a gfx950 device is present")
    with pytest.raises(ksim.KsimError) as ei:
        ksim.Engine(16, 1)
    assert ei.value.code == ksim.KSIM_ENODEV


def test_product_does_not_reference_oracle():
    # the product library must not link or name anything under oracle/
    out = subprocess.run(["nm", "-D", ksim.LIB_PATH], capture_output=True, text=True).stdout
    assert "orc_" not in out
    deps = subprocess.run(["ldd", ksim.LIB_PATH], capture_output=True, text=True).stdout
    assert "oracle" not in deps
    for root, _, files in os.walk(ksim.PKG_DIR):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".hpp", ".h")):
                txt = open(os.path.join(root, f)).read()
                assert "pyoracle" not in txt and "liboracle" not in txt, f


def test_integration_names_every_entry_point():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    missing = sorted(n for n in declared_functions() if "`" + n + "`" not in doc and "C." + n not in doc)
    assert not missing, missing


GO_SHIM = os.path.join(ROOT, "go", "ksim_gpu.go")


def test_go_shim_binds_only_declared_symbols():
    # go/ksim_gpu.go (the cgo plugin, source only: no Go toolchain here) calls only what include/*.h
    # declares, uses every plugin-level entry point, and implements the framework methods it registers
    src = open(GO_SHIM).read()
    used = set(re.findall(r"C\.(ksim_[a-z_0-9]+)\(", src))
    assert used and used <= declared_functions(), sorted(used - declared_functions())
    for n in ("ksim_engine_create", "ksim_engine_set_nodes", "ksim_engine_set_typical", "ksim_engine_set_policy",
              "ksim_engine_filter_score", "ksim_engine_reserve", "ksim_engine_unreserve", "ksim_engine_bind",
              "ksim_engine_set_power_model", "ksim_engine_destroy"):
        assert n in used, n
    for m in ("PreFilter", "PreFilterExtensions", "Filter", "Score", "ScoreExtensions", "NormalizeScore", "Reserve",
              "Unreserve", "Name"):
        assert re.search(r"func \(p \*KsimGpuPlugin\) %s\(" % m, src), m
    # the helpers the r1 sketch left undefined are defined here
    for f in ("typeMask", "typeID", "toKsimPod", "gpuIndexString", "maskFromGpuIndexAnnotation", "affinityTag",
              "ensureEngine", "powerModel", "release"):
        assert re.search(r"func (\(p \*KsimGpuPlugin\) )?%s\(" % f, src), f
    # balanced braces / parens (a cheap syntax check in lieu of gofmt)
    code = re.sub(r'"(\\.|[^"\\])*"', '""', re.sub(r"//[^\n]*", "", src))
    assert code.count("{") == code.count("}") and code.count("(") == code.count(")")


def test_integration_points_to_go_shim():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "go/ksim_gpu.go" in doc
    assert "```go" not in doc  # the code lives in the file, not in the document


def test_library_built_from_this_tree():
    # the prebuilt libksim_hip.so travels to the GPU box untracked: it must be the build of these sources
    assert ksim.build_id() == ksim.source_hash(), "libksim_hip.so is stale: rebuild (make -C kubernetes-scheduler-simulator_amd)"
