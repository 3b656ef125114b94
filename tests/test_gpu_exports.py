"""libcbc_gpu.so is linked from several translation units (cbc_amd/csrc/cbc_gpu_internal.h): the functions they share lose
`static` and must stay hidden.  What the library exports is the C ABI and nothing else: its defined dynamic function symbols,
the functions include/cbc_gpu.h declares and gpu.EXPORTS are one set."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exported_functions(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, stdout=subprocess.PIPE, text=True).stdout
    # "T": code.  The other defined symbols are the kernels' handles and the code objects' ids (data), which the HIP runtime
    # looks up by name
    return {f[2] for f in (ln.split() for ln in out.splitlines()) if len(f) == 3 and f[1] in "Tt"}


def _declared_functions(header):
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    names = set()
    for m in re.finditer(r"^(?!static|typedef|#)[A-Za-z_][\w \t\*]*?\b(cbc_\w+)\s*\(", text, flags=re.M):
        names.add(m.group(1))
    return names


def test_library_exports_the_c_abi_and_nothing_else(built):
    from cbc_amd import gpu
    exported = _exported_functions(os.path.join(ROOT, "cbc_amd", "csrc", "libcbc_gpu.so"))
    declared = _declared_functions(os.path.join(ROOT, "include", "cbc_gpu.h"))
    assert len(gpu.EXPORTS) == len(set(gpu.EXPORTS))
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
    assert exported == set(gpu.EXPORTS), (sorted(exported - set(gpu.EXPORTS)), sorted(set(gpu.EXPORTS) - exported))
