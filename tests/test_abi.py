"""The C-ABI libraries load and export every symbol their headers declare; the ctypes
mirrors (each header's SIGNATURES / STRUCTS / CONSTANTS tables) agree with the compiled headers
field by field, constant by constant and parameter count by parameter count. No compute calls
(no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADERS = {"lgx.h": "liblgx.so", "lgx_mlp.h": "liblgx_mlp.so", "lgx_s8.h": "liblgx_s8.so"}

# Integer #defines of a header that its CONSTANTS table need not hold.
NOT_IN_CONSTANTS = {
    "LGX_ACT_NOISE_STREAM",  # mirrored by oracle/philox.py STREAM_ACT (compared below); the package never passes it
}


def _source(header):
    """The header without its comments."""
    src = open(os.path.join(REPO, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def _declared(header):
    return sorted(set(re.findall(r"\b(lgx_\w+)\s*\(", _source(header))) - {"lgx_gemm_args"})


def _defines(header):
    """{name: value} of the header's `#define LGX_* <integer>` lines."""
    pattern = r"^[ \t]*#[ \t]*define[ \t]+(LGX_\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$"
    return {n: int(v, 0) for n, v in re.findall(pattern, _source(header), flags=re.M)}


def _mirror(header):
    """The module that holds the header's SIGNATURES / STRUCTS / CONSTANTS."""
    from legged_gym_custom_amd import _abi, _abi_mlp
    from legged_gym_custom_amd.rsl_rl.modules import hip_s8
    return {"lgx.h": _abi, "lgx_mlp.h": _abi_mlp, "lgx_s8.h": hip_s8}[header]


def _field_names(cls):
    return [f[0] for f in cls._fields_]


@pytest.fixture(scope="module")
def libs():
    from legged_gym_custom_amd import build_native
    build_native.build()  # no-op when up to date (hipcc cross-compiles gfx950 here)
    return {h: C.CDLL(os.path.join(REPO, "legged_gym_custom_amd", "lib", lib)) for h, lib in HEADERS.items()}


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """What the three headers mean to g++ -std=c++17 (the host backend's compiler): one program prints
    sizeof of every struct in STRUCTS, offsetof / sizeof of every mirrored field and the value of every
    name in CONSTANTS. Returns {"S": {struct: size}, "F": {(struct, field): (offset, size)}, "C": {name: value}}."""
    lines = ["#include <cstddef>", "#include <cstdio>"] + [f'#include "{h}"' for h in sorted(HEADERS)]
    lines.append("int main() {")
    for header in sorted(HEADERS):
        m = _mirror(header)
        for cname, cls in m.STRUCTS.items():
            lines.append(f'  printf("S {cname} - %zu 0\\n", sizeof({cname}));')
            for field in _field_names(cls):
                lines.append(f'  printf("F {cname} {field} %zu %zu\\n", offsetof({cname}, {field}), '
                             f'sizeof((({cname}*)0)->{field}));')
        for name in list(m.CONSTANTS) + sorted(NOT_IN_CONSTANTS & set(_defines(header))):
            lines.append(f'  printf("C {name} - %lld 0\\n", (long long)({name}));')
    lines += ["  return 0;", "}"]
    d = tmp_path_factory.mktemp("abi_probe")
    src, exe = str(d / "probe.cpp"), str(d / "probe")
    with open(src, "w") as f:
        f.write("\n".join(lines) + "\n")
    cc = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(REPO, "include"), "-o", exe, src],
                        capture_output=True, text=True)
    assert cc.returncode == 0, "a mirror names something its header lacks:\n" + cc.stderr
    out = {"S": {}, "F": {}, "C": {}}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        kind, name, field, a, b = line.split()
        out[kind][(name, field) if kind == "F" else name] = (int(a), int(b)) if kind == "F" else int(a)
    return out


@pytest.mark.parametrize("header", sorted(HEADERS))
def test_every_declared_symbol_is_exported(libs, header):
    names = _declared(header)
    assert len(names) >= 4
    missing = [n for n in names if not hasattr(libs[header], n)]
    assert not missing, f"{HEADERS[header]} lacks {missing}"


def test_python_bindings_cover_the_headers():
    from legged_gym_custom_amd import _native
    from legged_gym_custom_amd.rsl_rl.modules import hip_mlp
    assert set(_declared("lgx.h")) == set(_native.EXPORTED)
    assert set(_declared("lgx_mlp.h")) == set(hip_mlp.EXPORTED)
    from legged_gym_custom_amd.rsl_rl.modules import hip_s8
    assert set(_declared("lgx_s8.h")) == set(hip_s8.EXPORTED)
    for header in HEADERS:  # the list is the table the loader applies, not a copy of it
        assert set(_declared(header)) == set(_mirror(header).SIGNATURES)


def test_struct_layouts_and_abi_versions(libs):
    from legged_gym_custom_amd import _abi, _native
    from legged_gym_custom_amd.rsl_rl.modules import hip_mlp
    L = _native.lib()  # checks abi version + lgx_sizeof_{model,task_params,buffers,eval_buffers}
    assert L.lgx_abi_version() == _abi.ABI_VERSION
    M = hip_mlp.lib()  # checks abi version + sizeof(lgx_gemm_args)
    assert M.lgx_mlp_sizeof_gemm_args() == C.sizeof(hip_mlp.GemmArgs)
    from legged_gym_custom_amd.rsl_rl.modules import hip_s8
    S8 = hip_s8.lib()  # checks abi version + sizeof(lgx_s8_{gemm,act_pack,chain,act}_args)
    assert S8.lgx_s8_sizeof_gemm_args() == C.sizeof(hip_s8.GemmArgs)


def test_gemm_rejects_bad_arguments_without_touching_the_device(libs):
    from legged_gym_custom_amd.rsl_rl.modules import hip_mlp
    L = hip_mlp.lib()
    a = hip_mlp.GemmArgs(M=-1, N=1, K=1)
    assert L.lgx_gemm(C.byref(a), None) < 0
    assert b"negative" in L.lgx_mlp_last_error()
    a = hip_mlp.GemmArgs(M=4, N=4, K=4, A=16, B=16, C=16, epilogue=hip_mlp.EPI_BIAS)
    assert L.lgx_gemm(C.byref(a), None) < 0 and b"bias" in L.lgx_mlp_last_error()
    assert L.lgx_mlp_pick_split(512, 627, 24576) >= 2


@pytest.mark.parametrize("header", sorted(HEADERS))
def test_every_header_struct_has_a_mirror(header):
    assert set(re.findall(r"\}\s*(lgx_\w+)\s*;", _source(header))) == set(_mirror(header).STRUCTS)


@pytest.mark.parametrize("header", sorted(HEADERS))
def test_field_layouts_match_the_compiled_header(compiled, header):
    wrong = []
    for cname, cls in _mirror(header).STRUCTS.items():
        if compiled["S"][cname] != C.sizeof(cls):
            wrong.append(f"sizeof({cname}): header {compiled['S'][cname]}, ctypes {C.sizeof(cls)}")
        for field in _field_names(cls):
            d = getattr(cls, field)
            if compiled["F"][(cname, field)] != (d.offset, d.size):
                wrong.append(f"{cname}.{field}: header (offset, size) {compiled['F'][(cname, field)]}, "
                             f"ctypes {(d.offset, d.size)}")
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("header", sorted(HEADERS))
def test_constants_match_the_compiled_header(compiled, header):
    constants = _mirror(header).CONSTANTS
    wrong = [f"{n}: header {compiled['C'][n]}, python {v}" for n, v in constants.items() if compiled["C"][n] != v]
    assert not wrong, "\n".join(wrong)
    unmirrored = set(_defines(header)) - set(constants) - NOT_IN_CONSTANTS
    assert not unmirrored, f"{header} defines {sorted(unmirrored)}: add them to the mirror's CONSTANTS"


def test_reward_ids_and_noise_stream(compiled):
    """enum lgx_reward_id is REWARD_IDS name by name; the act head's Philox stream is the oracle's."""
    import philox
    from legged_gym_custom_amd import _abi
    enumerators = set(re.findall(r"\bLGX_REW_\w+", _source("lgx.h")))
    assert enumerators == {"LGX_REW_" + n.upper() for n in _abi.REWARD_IDS} | {"LGX_REW_COUNT"}
    assert compiled["C"]["LGX_REW_COUNT"] == len(_abi.REWARD_IDS)
    assert compiled["C"]["LGX_ACT_NOISE_STREAM"] == philox.STREAM_ACT


@pytest.mark.parametrize("header", sorted(HEADERS))
def test_parameter_counts_match_the_header(header):
    decls = re.findall(r"\b(lgx_\w+)\s*\(([^()]*)\)\s*;", _source(header))
    signatures = _mirror(header).SIGNATURES
    assert {n for n, _ in decls} == set(signatures)
    wrong = []
    for name, params in decls:
        n = 0 if params.strip() in ("", "void") else params.count(",") + 1
        if n != len(signatures[name][1]):
            wrong.append(f"{name}: header {n} parameters, SIGNATURES {len(signatures[name][1])}")
    assert not wrong, "\n".join(wrong)
