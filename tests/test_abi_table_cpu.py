"""not-gpu: ``_native.PROTOTYPES`` against include/tac_amd.h — every declared function, every argument, every return type.

A width that disagrees with the header (``c_int32`` for an ``int64_t`` stride) does not fail a build: it truncates a value on its
way to a kernel.  The header is parsed here, so a declaration added or changed there fails this test until the table follows."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCALARS = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float,
           'double': ctypes.c_double}
DECLARATION = re.compile(r'^(?P<ret>[\w\s]+?\*?)\s*(?P<name>tac_\w+)\s*\((?P<args>[^()]*)\)$')
TYPEDEF = re.compile(r'typedef\s+struct\s+tac_stft_desc\s*\{(?P<body>[^}]*)\}\s*tac_stft_desc\s*;')


@pytest.fixture(scope='module')
def native():
    import torchaudio_contrib_amd as t
    if not os.path.exists(t._native.LIB_PATH):
        t.build_native()
    return t._native


@pytest.fixture(scope='module')
def header():
    """(statements outside the typedef, body of the typedef): comments and preprocessor lines gone"""
    text = open(os.path.join(ROOT, 'include', 'tac_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    text = '\n'.join(line for line in text.split('\n')
                     if not line.lstrip().startswith('#') and line.strip() not in ('extern "C" {', '}'))
    typedef = TYPEDEF.search(text)
    assert typedef is not None and len(TYPEDEF.findall(text)) == 1
    rest = text[:typedef.start()] + text[typedef.end():]
    return [' '.join(s.split()) for s in rest.split(';') if s.strip()], typedef.group('body')


def _equal(a, b):
    ints = (ctypes.c_int, ctypes.c_int32)                   # the one allowed equivalence
    return a is b or (a in ints and b in ints)


def _argument(text, native):
    if '*' in text:
        pointee = text[:text.index('*')].replace('const', ' ').split()
        assert len(pointee) == 1 and text.count('*') == 1, text
        return ctypes.POINTER(native.StftDesc) if pointee == ['tac_stft_desc'] else ctypes.c_void_p
    kind = text.split()[:-1]                                # (the last word is the parameter's name)
    assert len(kind) == 1 and kind[0] in SCALARS, 'unknown C type in %r' % text
    return SCALARS[kind[0]]


def _declared(header, native):
    found = {}
    for statement in header[0]:
        m = DECLARATION.match(statement)
        assert m is not None, 'not a tac_* declaration: %r' % statement
        ret = ' '.join(m.group('ret').split())
        if ret in ('const char*', 'const char *'):
            restype = ctypes.c_char_p
        else:
            assert ret in SCALARS, 'unknown C return type in %r' % statement
            restype = SCALARS[ret]
        args = m.group('args').strip()
        argtypes = [] if args == 'void' else [_argument(a.strip(), native) for a in args.split(',')]
        assert m.group('name') not in found, m.group('name')
        found[m.group('name')] = (restype, argtypes)
    return found


def test_table_names_are_the_headers(header, native):
    declared = _declared(header, native)
    assert len(declared) >= 116
    assert set(declared) == set(native.PROTOTYPES)
    assert native.EXPORTS == tuple(native.PROTOTYPES)


def test_every_prototype_matches_its_declaration(header, native):
    for name, (restype, argtypes) in _declared(header, native).items():
        table_restype, table_argtypes = native.PROTOTYPES[name]
        assert _equal(table_restype, restype), (name, table_restype, restype)
        assert len(table_argtypes) == len(argtypes), (name, len(table_argtypes), len(argtypes))
        for i, (got, want) in enumerate(zip(table_argtypes, argtypes)):
            assert _equal(got, want), (name, i, got, want)


def test_parser_refuses_what_it_does_not_know(native):
    with pytest.raises(AssertionError, match='unknown C type'):
        _argument('uint16_t flags', native)
    with pytest.raises(AssertionError, match='unknown C return type'):
        _declared((['size_t tac_bytes(void)'], ''), native)
    with pytest.raises(AssertionError, match='not a tac_'):
        _declared((['int other_function(int x)'], ''), native)
    assert _argument('int64_t stride_r', native) is ctypes.c_int64 and not _equal(ctypes.c_int64, ctypes.c_int32)


def test_stft_desc_mirrors_the_typedef(header, native):
    fields = re.findall(r'\b(int64_t|int32_t)\s+(\w+)\s*;', header[1])
    assert len(fields) == len([s for s in header[1].split(';') if s.strip()])          # nothing in the body was passed over
    assert [kind for kind, _ in fields] == ['int64_t'] * 3 + ['int32_t'] * 8
    assert [(name, SCALARS[kind]) for kind, name in fields] == [(f[0], f[1]) for f in native.StftDesc._fields_]
    assert ctypes.sizeof(native.StftDesc) == 3 * 8 + 8 * 4


def test_loaded_library_carries_the_table(native):
    h = native.lib()
    for name, (restype, argtypes) in native.PROTOTYPES.items():
        fn = getattr(h, name)                               # (AttributeError: the library does not export it)
        assert fn.restype is restype, name
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name
