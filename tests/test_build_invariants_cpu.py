"""Source-level invariants of the HIP kernels that the compiler does not enforce.

Dynamic LDS (``extern __shared__``) starts right after a kernel's static LDS segment, aligned only to the declared
type: a float array after a 1,720-byte static segment began at 8 mod 16 bytes, and every ``ds_read_b128`` of the
MLP rollout kernel's weights and activations was misaligned (its 128 x 128 layer ran at 8-9 k instead of ~2.5 k
shader cycles; profiles/r2_probe_mfma_f32_rate.txt). Every dynamic LDS array must therefore be declared 16-byte
aligned."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dynamic_lds_arrays_are_16_byte_aligned():
    offenders = []
    for path in glob.glob(os.path.join(ROOT, "csrc", "kernels", "*.hip")) + \
            glob.glob(os.path.join(ROOT, "csrc", "kernels", "*.h")):
        for i, line in enumerate(open(path), 1):
            if re.search(r"extern\s+__shared__", line) and "aligned(16)" not in line:
                offenders.append(f"{os.path.basename(path)}:{i}: {line.strip()}")
    assert not offenders, offenders


def test_no_cuda_compat_layers():
    """CDNA4 code only: no CUDA shims, hipify markers or dual-platform paths in the kernels."""
    bad = []
    for path in glob.glob(os.path.join(ROOT, "csrc", "**", "*.*"), recursive=True):
        if not path.endswith((".hip", ".h", ".cpp")):
            continue
        txt = open(path, errors="ignore").read()
        for pat in ("__HIP_PLATFORM_NVIDIA__", "#include <cuda", "cudaStream_t", "__CUDA_ARCH__"):
            if pat in txt:
                bad.append((os.path.basename(path), pat))
    assert not bad, bad


def test_fused_head_gate_matches_kernel_limits():
    """the Python gate of the fused A2C head (engine.head_ok) applies the same limits as the kernel's
    launcher (loss.hip aca_head_bwd: B <= 512 rows, N <= 256 envs, 2..7 actions), so e.g. n_steps=1 with 300 envs
    takes the loss + GEMM path instead of failing at launch."""
    from actor_critic_algs_on_tensorflow_amd.algos.engine import CNNEngine
    eng = CNNEngine.__new__(CNNEngine)
    eng.fused_head, eng.A = True, 6
    assert eng.head_ok(160, 32)
    assert eng.head_ok(512, 256)
    assert not eng.head_ok(300, 300)     # one step of 300 envs: N > 256
    assert not eng.head_ok(640, 128)     # B > 512
    eng.A = 8
    assert not eng.head_ok(160, 32)
    src = open(os.path.join(ROOT, "csrc", "kernels", "loss.hip")).read()
    assert "B > aca::HB_MAXB || N > 256" in src and "constexpr int HB_MAXB = 512;" in src


# ---- the C launcher interface is declared once (csrc/kernels/launch_api.h) and included by both sides, so the
# compiler checks every aca_* definition and call against it (C-linkage functions cannot be overloaded)
API = "launch_api.h"
_NOT_TYPES = {"return", "else", "case", "throw", "new", "delete", "goto", "sizeof"}


def _csrc_sources():
    out = {}
    for path in glob.glob(os.path.join(ROOT, "csrc", "**", "*.*"), recursive=True):
        if path.endswith((".hip", ".h", ".cpp")):
            txt = open(path, errors="ignore").read()
            txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
            txt = re.sub(r"//[^\n]*", " ", txt)
            txt = re.sub(r"(?m)^[ \t]*#.*(?:\\\n.*)*$", " ", txt)      # preprocessor lines (macro bodies included)
            out[os.path.relpath(path, os.path.join(ROOT, "csrc"))] = txt
    return out


def _aca_entities(txt):
    """(name, kind) of every aca_* function declared ('decl': the parameter list is followed by ';' and the text in
    front of the name is a return type, not an expression) or defined ('def': followed by '{') in txt."""
    found = []
    for m in re.finditer(r"\baca_\w+\s*\(", txt):
        depth, j = 1, m.end()
        while depth and j < len(txt):
            depth += {"(": 1, ")": -1}.get(txt[j], 0)
            j += 1
        tail = txt[j:].lstrip()[:1]
        start = max(txt.rfind(c, 0, m.start()) for c in ";{}") + 1
        head = txt[start:m.start()].replace('extern "C"', " ")
        words = re.findall(r"[A-Za-z_]\w*", head)
        is_type = bool(words) and re.fullmatch(r"[\w\s:\*&]+", head) is not None and not (set(words) & _NOT_TYPES)
        if is_type and tail == ";":
            found.append((m.group(0).rstrip("( \t\n"), "decl"))
        elif is_type and tail == "{":
            found.append((m.group(0).rstrip("( \t\n"), "def"))
    return found


def test_launchers_are_declared_only_in_the_shared_header():
    stray = []
    for rel, txt in _csrc_sources().items():
        if os.path.basename(rel) == API:
            continue
        stray += [f"{rel}: {name}" for name, kind in _aca_entities(txt) if kind == "decl"]
    assert not stray, stray


def test_every_launcher_definition_sees_the_shared_header():
    src = _csrc_sources()
    missing = []
    for rel, txt in src.items():
        if rel.endswith(".hip") and any(kind == "def" for _, kind in _aca_entities(txt)):
            raw = open(os.path.join(ROOT, "csrc", rel)).read()
            if f'#include "{API}"' not in raw:
                missing.append(rel)
    assert not missing, missing
    assert f'#include "{API}"' in open(os.path.join(ROOT, "csrc", "bindings.cpp")).read()


def test_declared_and_defined_launchers_agree():
    src = _csrc_sources()
    declared = [n for n, kind in _aca_entities(src[os.path.join("kernels", API)]) if kind == "decl"]
    assert len(declared) > 50 and len(set(declared)) == len(declared), "every entry point is declared once"
    defined = {}
    for rel, txt in src.items():
        if rel.endswith(".hip"):
            for name, kind in _aca_entities(txt):
                if kind == "def":
                    defined.setdefault(name, []).append(rel)
    assert not {n: f for n, f in defined.items() if len(f) != 1}, "an entry point is defined in exactly one .hip file"
    assert set(declared) == set(defined), (sorted(set(declared) - set(defined)), sorted(set(defined) - set(declared)))
