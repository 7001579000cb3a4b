"""The one reader of include/pcbenv.h for the tests: the text as written, the text without comments, and what it declares --
every function prototype and every `typedef struct` -- with C types normalised to single spaces and each `*` written
against what follows it ("const int32_t *", "pcbenv **", "pcbenv_instgen *const *")."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(REPO, "include", "pcbenv.h")

_STRUCT = r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;"


def raw() -> str:
    """include/pcbenv.h as written."""
    with open(PATH) as f:
        return f.read()


def text() -> str:
    """include/pcbenv.h with the comments stripped."""
    return re.sub(r"/\*.*?\*/", "", raw(), flags=re.S)


def _ctype(tokens) -> str:
    out = ""
    for t in tokens:
        out += ("" if not out or out.endswith("*") else " ") + t
    return out


def _declarator(decl: str):
    """`const int32_t *actions_dev` -> ("const int32_t *", "actions_dev")."""
    tokens = re.findall(r"\w+|\*", decl)
    assert len(tokens) >= 2 and re.fullmatch(r"[A-Za-z_]\w*", tokens[-1]), decl
    return _ctype(tokens[:-1]), tokens[-1]


def prototypes():
    """[(return type, name, [(C type, parameter name), ...]), ...] in the order of the header; `(void)` is no parameter."""
    body = re.sub(_STRUCT, "", text(), flags=re.S)
    body = re.sub(r"\benum\s+\w+\s*\{.*?\}\s*;", "", body, flags=re.S)
    body = re.sub(r"^\s*#.*$", "", body, flags=re.M)
    body = re.sub(r'extern\s+"C"\s*\{|\btypedef\s+struct\s+\w+\s+\w+\s*;', "", body)
    out = []
    for statement in body.split(";"):
        m = re.fullmatch(r"\s*([\w\s\*]+?)\s*\b(\w+)\s*\(([^()]*)\)\s*", statement, flags=re.S)
        if not m:
            assert not statement.strip(" \n}"), f"not a prototype: {statement.strip()!r}"
            continue
        params = [] if m.group(3).strip() == "void" else [_declarator(p) for p in m.group(3).split(",")]
        out.append((_ctype(re.findall(r"\w+|\*", m.group(1))), m.group(2), params))
    return out


def declared_functions():
    """The names of the functions the header declares, sorted."""
    return sorted({name for _, name, _ in prototypes()})


def structs():
    """{struct name: [(C type, member name), ...]} for every `typedef struct`; `int32_t *a, *b;` is two members."""
    out = {}
    for name, body in re.findall(_STRUCT, text(), flags=re.S):
        members = []
        for decl in filter(str.strip, body.split(";")):
            base = re.match(r"\s*((?:const\s+)?\w+)", decl)
            for item in decl[base.end():].split(","):
                ctype, member = _declarator(base.group(1) + " " + item)
                members.append((ctype, member))
        out[name] = members
    return out
