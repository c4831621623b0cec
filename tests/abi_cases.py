"""What every table of entry points of restartsqp_amd/capi.py owes the header under include/ that declares them, and what a struct
of the binding owes the header's struct: the checks the *_args tests share. Needs the built library and no GPU."""
import ctypes as C
import os
import re

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
RETURNS = {C.c_int: "int", C.c_double: "double", C.c_float: "float", C.c_char_p: "const char *", None: "void"}
ELEMENTS = {"int32": "int", "float64": "double"}


def header(name):
    return open(os.path.join(INCLUDE, name)).read()


def uncommented(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def declared(text):
    """{entry point: return type} of the declarations in a header's text, comments aside"""
    return {name: ret.strip() for ret, name in re.findall(r"^[ \t]*(const char \*|(?:int|void|double|float)\s+)(rsqp_\w+)\s*\(",
                                                          uncommented(text), flags=re.M)}


def assert_entry_points(capi, name, table, expected, structs=()):
    """the header `name` declares exactly the entry points `expected`, each with the return type `table` binds; `table` is the
    registry's table of that header and holds exactly them; the library exports each with the table's types bound; no other table
    and no other header names one of them; rsqp_hip.h includes the header; and each (C struct, binding class) of `structs` agrees
    (assert_struct). Returns the header's text"""
    text = header(name)
    assert name == "rsqp_hip.h" or re.search(r'^#include "%s"' % re.escape(name), header("rsqp_hip.h"), flags=re.M), name
    assert capi.SYMBOL_TABLES[name] is table
    decl = declared(text)
    assert set(decl) == set(table) == set(expected), set(decl) ^ set(table) | set(table) ^ set(expected)
    L = capi.lib()
    for fn in expected:
        res, args = table[fn]
        assert decl[fn] == RETURNS[res] and re.search(r"\b%s\s*%s\s*\(" % (re.escape(RETURNS[res]), fn), text), fn
        assert hasattr(L, fn), "librsqp_hip.so does not export %s" % fn
        assert getattr(L, fn).argtypes == args and getattr(L, fn).restype is res, fn
    for other, t in capi.SYMBOL_TABLES.items():
        assert t is table or not set(expected) & set(t), (other, set(expected) & set(t))
    for other in sorted(os.listdir(INCLUDE)):
        if other != name:
            # an extension's entry points are not even spoken of as calls elsewhere ("fn (the header that declares it)" is a reference,
            # not a call); those of rsqp_hip.h are, in the extensions' comments
            there = header(other) if name != "rsqp_hip.h" else uncommented(header(other))
            for fn in expected:
                assert not re.search(r"\b%s\s*\((?!%s\))" % (fn, re.escape(name)), there), (other, fn)
    for struct, cls in structs:
        assert_struct(text, struct, cls)
    return text


def assert_struct(text, struct, cls):
    """the binding's class has the fields of the header's struct, in order; for a struct of pointers to pooled arguments also row by
    row of its table: the element type is the header's (int * / double *), the role is "in" exactly where the header says const, and
    IN / INOUT / OUT / INTS are the table filtered in order"""
    body = uncommented(re.search(r"typedef struct \{([^{}]*)\} %s;" % struct, text).group(1))
    assert re.findall(r"[\s*](\w+)\s*[,;]", body) == [k for k, _ in cls._fields_], struct
    if not hasattr(cls, "ROWS"):
        return
    fields = []
    for line in filter(None, (ln.strip() for ln in body.splitlines())):
        const, element, names = re.fullmatch(r"(const )?(int|double) (\*\w+(?:, \*\w+)*);", line).groups()
        fields += [(k.lstrip("*"), bool(const), element) for k in names.split(", ")]
    assert fields == [(k, role == "in", ELEMENTS[dtype]) for k, role, length, dtype in cls.ROWS], struct
    assert all(t is C.c_void_p for _, t in cls._fields_)
    assert {role for _, role, _, _ in cls.ROWS} <= {"in", "inout", "out"} and {length for _, _, length, _ in cls.ROWS} <= {"nq", "sN", "sC"}
    for tup, keep in (("IN", lambda r: r[1] == "in"), ("INOUT", lambda r: r[1] == "inout"), ("OUT", lambda r: r[1] == "out"),
                      ("INTS", lambda r: r[3] == "int32")):
        assert getattr(cls, tup) == tuple(r[0] for r in cls.ROWS if keep(r)), (struct, tup)
    assert set(cls.IN + cls.INOUT + cls.OUT) == {k for k, _ in cls._fields_}
