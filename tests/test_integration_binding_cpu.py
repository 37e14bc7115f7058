"""INTEGRATION.md's Rust binding against what it binds: every function of its `extern "C"` blocks is declared in
include/zkvm_gpu.h with the same parameters in the same order, every `#[repr(C)]` struct has the header struct's fields
in the header's order and the size of the ctypes structure in zkvm_amd/native.py, and -- where the reference's
sources are at hand -- every `server_key.<method>(` the snippets call is a method of fhe/src/server_key.rs."""
import ctypes as C
import os
import re
from pathlib import Path

import pytest

from zkvm_amd import native

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "zkvm_gpu.h").read_text()
DOC = (ROOT / "INTEGRATION.md").read_text()
SERVER_KEY_RS = Path(os.environ.get("ZKVM_REFERENCE_DIR", "/root/reference")) / "fhe" / "src" / "server_key.rs"

RUST_BLOCKS = re.findall(r"```rust\n(.*?)```", DOC, flags=re.S)
# Rust struct -> (header struct, ctypes structure)
STRUCTS = {"ZkOptions": ("zk_options", native.Options), "ZkPubInputs": ("zk_pub_inputs", native.PubInputs),
           "ZkProofInfo": ("zk_proof_info", native.ProofInfo), "ZkJobResult": ("zk_job_result", native.JobResult)}
RUST_SIZES = {"u8": 1, "i8": 1, "c_char": 1, "u32": 4, "i32": 4, "f32": 4, "c_int": 4, "u64": 8, "i64": 8, "f64": 8,
              "usize": 8}


def strip_comments(text: str) -> str:
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def split_top(text: str, sep: str = ","):
    """Split at `sep` outside brackets."""
    out, depth, cur = [], 0, ""
    for ch in text:
        depth += ch in "([{<"
        depth -= ch in ")]}>"
        if ch == sep and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += ch
    return [p.strip() for p in out + [cur] if p.strip()]


def rust_functions():
    """{name: [(parameter, is_pointer)]} over every extern "C" block of the document."""
    fns = {}
    for block in RUST_BLOCKS:
        for ext in re.findall(r'extern "C" \{([^}]*)\}', strip_comments(block)):
            for name, params in re.findall(r"\bfn\s+(\w+)\s*\((.*?)\)\s*(?:->[^;]*)?;", ext, flags=re.S):
                got = []
                for p in split_top(params):
                    pname, ptype = p.split(":", 1)
                    got.append((pname.strip().rstrip("_"), ptype.strip().startswith("*")))
                assert fns.setdefault(name, got) == got, f"{name} is declared twice, differently"
    return fns


def header_prototype(name: str):
    m = re.search(r"\b(?:int|void|const char \*)\s*" + name + r"\s*\(([^;]*)\)\s*;", strip_comments(HEADER))
    if not m:
        return None
    params = m.group(1).strip()
    if params == "void":
        return []
    out = []
    for p in split_top(params):
        pname = re.search(r"(\w+)\s*(?:\[\d*\])*$", p).group(1)
        out.append((pname, "*" in p or "[" in p))
    return out


def header_struct(name: str):
    """[(field, array dimensions, C type)] of `typedef struct { ... } name;`."""
    m = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", strip_comments(HEADER))
    assert m, f"{name} is not a struct of include/zkvm_gpu.h"
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, rest = re.match(r"((?:const\s+)?\w+)\s+(.*)", decl, flags=re.S).groups()
        for item in rest.split(","):
            fname, dims = re.match(r"\s*(\w+)((?:\[\w+\])*)", item).groups()
            fields.append((fname, [int(d) for d in re.findall(r"\[(\d+)\]", dims)], ctype))
    return fields


def rust_structs():
    """{name: [(field, rust type)]} over every #[repr(C)] struct of the document (opaque handles have one `_p`)."""
    out = {}
    for block in RUST_BLOCKS:
        for name, body in re.findall(r"#\[repr\(C\)\]\s*pub struct (\w+)\s*\{(.*?)\}", strip_comments(block), flags=re.S):
            fields = [tuple(s.strip() for s in f.replace("pub ", "", 1).split(":", 1)) for f in split_top(body)]
            assert out.setdefault(name, fields) == fields, f"{name} is defined twice, differently"
    return out


def rust_size(rtype: str, structs) -> tuple:
    """(size, array dimensions outermost first) of a Rust field type."""
    m = re.match(r"\[(.*);\s*(\d+)\]$", rtype)
    if m:
        size, dims = rust_size(m.group(1).strip(), structs)
        return size * int(m.group(2)), [int(m.group(2))] + dims
    if rtype in RUST_SIZES:
        return RUST_SIZES[rtype], []
    return sum(rust_size(t, structs)[0] for _, t in structs[rtype]), []  # (the nested structs here have no padding)


def test_the_document_has_the_blocks_the_test_reads():
    fns, structs = rust_functions(), rust_structs()
    assert len(RUST_BLOCKS) >= 8 and len(fns) >= 30
    for name in ("zk_prove_columns", "zk_vm_prove", "zk_queue_create", "zk_queue_submit_vm", "zk_queue_wait",
                 "zk_queue_wait_any"):
        assert name in fns, name
    assert set(STRUCTS) <= set(structs)


@pytest.mark.parametrize("name", sorted(rust_functions()))
def test_extern_function_matches_the_header(name):
    want = header_prototype(name)
    assert want is not None, f"INTEGRATION.md binds {name}, which include/zkvm_gpu.h does not declare"
    got = rust_functions()[name]
    assert [p for p, _ in got] == [p for p, _ in want], f"{name}: parameters differ from the header's"
    assert [ptr for _, ptr in got] == [ptr for _, ptr in want], f"{name}: a pointer on one side is a value on the other"


@pytest.mark.parametrize("name", sorted(rust_structs()))
def test_repr_c_struct_matches_the_header_and_ctypes(name):
    structs = rust_structs()
    fields = structs[name]
    if [f for f, _ in fields] == ["_p"]:
        assert fields[0][1] == "[u8; 0]"  # an opaque handle
        return
    assert name in STRUCTS, f"INTEGRATION.md defines {name}: add its header struct and ctypes structure to STRUCTS"
    cname, ctype = STRUCTS[name]
    want = header_struct(cname)
    assert [f for f, _ in fields] == [f for f, _, _ in want], f"{name}: fields differ from {cname}'s"
    total = 0
    for (fname, rtype), (_, dims, _) in zip(fields, want):
        size, rdims = rust_size(rtype, structs)
        assert rdims == dims, f"{name}.{fname}: array shape {rdims}, the header has {dims}"
        assert size == getattr(ctype, fname).size, f"{name}.{fname}: {size} bytes, ctypes has {getattr(ctype, fname).size}"
        assert total <= getattr(ctype, fname).offset < total + 8  # (alignment padding only)
        total = getattr(ctype, fname).offset + size
    assert (total + 7) // 8 * 8 == C.sizeof(ctype) or total == C.sizeof(ctype), f"{name}: size differs from ctypes"
    assert [f for f, _ in ctype._fields_] == [f for f, _ in fields]


def test_server_key_methods_exist_in_the_reference():
    called = set()
    for block in RUST_BLOCKS:
        called |= set(re.findall(r"\b(?:server_key|sk)\.(\w+)\(", strip_comments(block)))
    assert {"lwe_size", "encrypt_trivial"} <= called  # (the search found the calls)
    if not SERVER_KEY_RS.exists():
        pytest.skip("the reference's sources are not on this machine")
    defined = set(re.findall(r"\bpub fn (\w+)", SERVER_KEY_RS.read_text()))
    assert called <= defined, f"not public methods of ServerKey: {sorted(called - defined)}"
