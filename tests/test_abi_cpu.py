"""The C ABI and its Python mirror, checked as a whole and derived from what is there: every header of include/ compiles alone as
C99; every prototype of every header against the row of `_lib.HEADERS` under that header (names, arity, class of every parameter and
of the return type) and against what the loaded library was bound with; every field of every `ctypes.Structure` of `_lib` against
the C compiler's `offsetof` / `sizeof` and against the recorded table tests/golden/abi_layout_v6.json; every Python constant against
its `DLPM_*` twin; the build's source and header lists against the directories; the documents against the table.  Nothing here
names a feature: a new entry point is a prototype in a header plus its row in `_lib.HEADERS`, and this file picks both up.

    python tests/test_abi_cpu.py --record      # writes the recorded layout table (only with a new ABI_VERSION)
"""
import ctypes as C
import inspect
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from dlpm_amd import _lib, build, datasets, metrics

INCLUDE = os.path.join(ROOT, 'include')
HEADERS = sorted(f for f in os.listdir(INCLUDE) if f.endswith('.h'))
MIRRORS = [v for v in vars(_lib).values() if isinstance(v, type) and issubclass(v, C.Structure)]
LAYOUT_FILE = os.path.join(ROOT, 'tests', 'golden', 'abi_layout_v%d.json' % _lib.ABI_VERSION)
GCC = ['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I', INCLUDE]
SCALARS = {'int': C.c_int32, 'int32_t': C.c_int32, 'int64_t': C.c_int64, 'uint32_t': C.c_uint32, 'uint64_t': C.c_uint64,
           'float': C.c_float, 'double': C.c_double}
# bound functions INTEGRATION.md does not name, as of the commit that added this file: the set may only shrink
UNDOCUMENTED = {
    'dlpm_abi_version', 'dlpm_prof_enable', 'dlpm_prof_report', 'dlpm_mt19937_seed', 'dlpm_skewed_levy_host_f32',
    'dlpm_randn_host_f32', 'dlpm_skewed_levy_philox_f32', 'dlpm_skewed_levy_elem_philox_f32', 'dlpm_init_state_elem_philox_f32',
    'dlpm_init_state_philox_f32', 'dlpm_coeff_tables_f32', 'dlpm_fill_scaled_t_f32', 'dlpm_scale_by_table_f32',
    'dlpm_lim_tables_f32', 'dlpm_lim_update_f32', 'dlpm_fill_table_t_f32', 'dlpm_at_t_f32', 'dlpm_png_bound',
    'dlpm_png_encode_rgb8', 'dlpm_unet_num_classes', 'dlpm_unet_num_params', 'dlpm_unet_param_key',
    'dlpm_unet_time_embedding_width', 'dlpm_unet_time_embeddings_scratch_bytes', 'dlpm_unet_keep_features',
    'dlpm_unet_num_features', 'dlpm_unet_feature_shape', 'dlpm_unet_get_feature', 'dlpm_unet_flops_per_sample',
    'dlpm_unet_destroy', 'dlpm_mlp_destroy', 'dlpm_groupnorm_coeffs_f32', 'dlpm_attention_general_f32',
    'dlpm_timestep_embedding_f32', 'dlpm_nchw_to_nhwc_f32', 'dlpm_nhwc_to_nchw_f32', 'dlpm_sampler_begin_injected',
    'dlpm_sampler_step_injected', 'dlpm_sampler_state', 'dlpm_sampler_t', 'dlpm_sampler_table', 'dlpm_sampler_destroy',
    'dlpm_mlp_grad_param_floats', 'dlpm_mlp_grad_export_params_f32', 'dlpm_mlp_grad_import_params_f32',
    'dlpm_mlp_grad_workspace_bytes',
}


# ------------------------------------------------------------------------------------------ reading the headers
def code_of(header):
    """The header without comments, preprocessor lines and the extern "C" opening."""
    text = open(os.path.join(INCLUDE, header)).read().replace('\\\n', ' ')
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    text = re.sub(r'^[ \t]*#[^\n]*', ' ', text, flags=re.M)
    return re.sub(r'extern\s+"C"\s*\{', ' ', text)


def prototypes(header):
    """{name: (return type, [parameter declarations])} of every function the header declares, struct and enum bodies removed."""
    code, n = code_of(header), 1
    while n:
        code, n = re.subn(r'\{[^{}]*\}', ' ', code)
    found = {}
    for ret, name, params in re.findall(r'([A-Za-z_][\w\s\*]*?)\b(dlpm_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', code):
        assert name not in found, '%s declares %s twice' % (header, name)
        params = [p.strip() for p in params.split(',')]
        found[name] = (' '.join(ret.split()), [] if params == ['void'] else params)
    return found


def constants(header):
    """Names of the enumerators and of the object-like macros with a value (the include guard has none) that the header defines."""
    raw = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    names = set(re.findall(r'^[ \t]*#[ \t]*define[ \t]+(DLPM_[A-Z0-9_]+)[ \t]+\S', raw, flags=re.M))
    for enum in enums(header).values():
        names |= set(enum)
    return names


def enums(header):
    """{enum tag: [enumerators in order]}"""
    return {tag: [e.split('=')[0].strip() for e in body.split(',') if e.strip()]
            for tag, body in re.findall(r'\benum\s+(\w+)\s*\{([^{}]*)\}', code_of(header))}


def c_class(decl, header):
    """What a parameter or return declaration is at the ABI: 'void', 'char*', 'ptr' or the ctypes scalar."""
    if '*' in decl or '[' in decl:
        return 'char*' if re.match(r'(const\s+)?char\s*\*', decl) else 'ptr'
    words = [w for w in re.findall(r'\w+', decl) if w != 'const']
    if words[0] in ('void', 'dlpm_stream_t'):
        return 'void' if words[0] == 'void' else 'ptr'
    assert words[0] in SCALARS, '%s: no ctypes class is known for "%s"' % (header, decl)
    return SCALARS[words[0]]


def py_class(t):
    if t is None:
        return 'void'
    if t is C.c_char_p:
        return 'char*'
    return 'ptr' if t is C.c_void_p or issubclass(t, C._Pointer) else t


def same_class(c, p):
    return c == p or (c == 'char*' and p == 'ptr') or (c == 'ptr' and p == 'char*')


# ------------------------------------------------------------------------------------------ headers and prototypes
@pytest.mark.parametrize('header', HEADERS)
def test_header_compiles_alone_as_c99(header, tmp_path):
    src = tmp_path / 'alone.c'
    src.write_text('#include "%s"\n' % header)
    subprocess.check_call(GCC + ['-fsyntax-only', str(src)])
    assert header == 'dlpm_amd.h' or '#include "dlpm_amd.h"' in open(os.path.join(INCLUDE, header)).read()


def test_one_table_row_group_per_header():
    assert list(_lib.HEADERS) and sorted(_lib.HEADERS) == HEADERS
    assert sum(len(t) for t in _lib.HEADERS.values()) == len(_lib.SIGNATURES) > 0          # no name under two headers


@pytest.mark.parametrize('header', HEADERS)
def test_prototypes_match_the_table(header):
    declared, bound = prototypes(header), _lib.HEADERS[header]
    assert declared, 'no prototype found in ' + header
    assert set(declared) == set(bound), '%s: declared but not bound %s, bound but not declared %s' % (
        header, sorted(set(declared) - set(bound)), sorted(set(bound) - set(declared)))
    bad = []
    for name, (ret, params) in declared.items():
        res, args = bound[name]
        if len(params) != len(args):
            bad.append('%s: %d parameters in %s, %d argtypes' % (name, len(params), header, len(args)))
            continue
        # a returned `const char *` is c_char_p and nothing else: ctypes converts it
        if c_class(ret, header) != py_class(res):
            bad.append('%s: returns "%s" in %s, restype is %s' % (name, ret, header, getattr(res, '__name__', res)))
        for i, (decl, a) in enumerate(zip(params, args)):
            if not same_class(c_class(decl, header), py_class(a)):
                bad.append('%s: parameter %d is "%s" in %s, argtypes[%d] is %s' % (name, i, decl, header, i, a.__name__))
    assert not bad, '\n'.join(bad)
    print('%s: %d prototypes' % (header, len(declared)))


def test_the_loaded_library_is_bound_with_the_table():
    L = _lib.lib()                                                      # getattr fails on a missing export
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert L.dlpm_abi_version() == _lib.ABI_VERSION == 6
    assert len(_lib.SIGNATURES) == sum(len(prototypes(h)) for h in HEADERS) > 0
    print('%d functions bound' % len(_lib.SIGNATURES))


# ------------------------------------------------------------------------------------------ layouts and constants: one C program
def python_constants():
    """[(C name, Python value, where the value stands)] of every constant that mirrors a header."""
    pairs = [('DLPM_' + k, v, '_lib.' + k) for k, v in vars(_lib).items()
             if k.isupper() and type(v) is int and k != 'ABI_VERSION']
    pairs += [('DLPM_MEAN_' + k, v, '_lib.MEAN_TYPES[%r]' % k) for k, v in _lib.MEAN_TYPES.items()]
    pairs += [('DLPM_CONV_FAMILY_' + k, i, '_lib.CONV_FAMILIES[%d]' % i) for i, k in enumerate(_lib.CONV_FAMILIES)]
    pairs += [('DLPM_TOY_' + k.upper(), v, 'datasets.KINDS[%r]' % k) for k, v in datasets.KINDS.items()]
    defined = set().union(*(constants(h) for h in HEADERS))
    pairs += [('DLPM_' + k, v, 'metrics.' + k) for k, v in vars(metrics).items()
              if k.isupper() and type(v) is int and 'DLPM_' + k in defined]
    return pairs + [('DLPM_ERR_ARG', -1, 'the status _lib.check raises ValueError for')]


def run_probe(tmp):
    """Compile and run the program that prints every mirrored struct's layout and every mirrored constant."""
    lines = ['#include <stddef.h>', '#include <stdio.h>'] + ['#include "%s"' % h for h in HEADERS] + ['int main(void) {']
    for S in MIRRORS:
        c = S._c_name_
        lines.append('printf("S %s %%zu\\n", sizeof(%s));' % (c, c))
        for f, _ in S._fields_:
            lines.append('printf("F %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (c, f, c, f, c, f))
    for c, _, _ in python_constants():
        lines.append('printf("K %s %%lld\\n", (long long)%s);' % (c, c))
    src, exe = os.path.join(tmp, 'probe.c'), os.path.join(tmp, 'probe')
    open(src, 'w').write('\n'.join(lines + ['return 0; }', '']))
    subprocess.check_call(GCC + [src, '-o', exe])
    layout, values = {}, {}
    for w in (line.split() for line in subprocess.check_output([exe], text=True).splitlines()):
        if w[0] == 'S':
            layout[w[1]] = {'size': int(w[2]), 'fields': {}}
        elif w[0] == 'F':
            layout[w[1]]['fields'][w[2]] = [int(w[3]), int(w[4])]
        else:
            values[w[1]] = int(w[2])
    return layout, values


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
    for S in MIRRORS:
        assert getattr(S, '_c_name_', None), '%s does not name its C type in _c_name_' % S.__name__
    for c, _, where in python_constants():
        assert any(c in constants(h) for h in HEADERS), '%s has no twin %s in a header of include/' % (where, c)
    return run_probe(str(tmp_path_factory.mktemp('abi')))


def ctypes_layout():
    return {S._c_name_: {'size': C.sizeof(S), 'fields': {f: [getattr(S, f).offset, getattr(S, f).size] for f, _ in S._fields_}}
            for S in MIRRORS}


def layout_differences(a, b, a_name, b_name):
    bad = ['struct %s is in %s only' % (s, a_name if s in a else b_name) for s in sorted(set(a) ^ set(b))]
    for s in sorted(set(a) & set(b)):
        if a[s]['size'] != b[s]['size']:
            bad.append('sizeof(%s): %d in %s, %d in %s' % (s, a[s]['size'], a_name, b[s]['size'], b_name))
        fa, fb = a[s]['fields'], b[s]['fields']
        if list(fa) != list(fb):
            bad.append('%s: fields %s in %s, %s in %s' % (s, [f for f in fa if f not in fb] or list(fa), a_name,
                                                           [f for f in fb if f not in fa] or list(fb), b_name))
        bad += ['%s.%s: [offset, size] %s in %s, %s in %s' % (s, f, fa[f], a_name, fb[f], b_name)
                for f in fa if f in fb and fa[f] != fb[f]]
    return bad


def test_struct_layouts(probe):
    c_layout, py_layout = probe[0], ctypes_layout()
    bad = layout_differences(py_layout, c_layout, 'ctypes (_lib.py)', 'C (include/)')
    assert not bad, '\n'.join(bad)
    # every struct a header defines has a mirror (opaque handles have no body)
    defined = {n for h in HEADERS for n in re.findall(r'typedef\s+struct\s+\w+\s*\{[^{}]*\}\s*(\w+)\s*;', code_of(h))}
    assert defined == set(py_layout), defined ^ set(py_layout)
    recorded = json.load(open(LAYOUT_FILE))
    bad = layout_differences(c_layout, recorded, 'C (include/)', os.path.basename(LAYOUT_FILE))
    assert not bad, '\n'.join(bad + ['a struct layout is part of the ABI: a change needs a new _lib.ABI_VERSION / dlpm_abi_version() and '
                                     'a newly recorded tests/golden/abi_layout_v<N>.json (python tests/test_abi_cpu.py --record)'])
    n_fields = sum(len(s['fields']) for s in c_layout.values())
    assert len(c_layout) > 0 and n_fields > 0
    print('%d structs, %d fields, %d layout values' % (len(c_layout), n_fields, len(c_layout) + 2 * n_fields))


def test_constants(probe):
    pairs, values = python_constants(), probe[1]
    bad = ['%s is %d, %s is %d' % (where, v, c, values[c]) for c, v, where in pairs if values[c] != v]
    assert not bad, '\n'.join(bad)
    assert any(where == 'metrics.TAIL_MAX_LEVELS' for _, _, where in pairs)
    # the containers hold every enumerator of their enum, in its order
    tags = {tag: names for h in HEADERS for tag, names in enums(h).items()}
    assert tags['dlpm_mean_type'] == ['DLPM_MEAN_' + k for k in _lib.MEAN_TYPES]
    assert tags['dlpm_conv_family'] == ['DLPM_CONV_FAMILY_' + k for k in _lib.CONV_FAMILIES]
    assert tags['dlpm_toy_kind'] == ['DLPM_TOY_' + k.upper() for k in datasets.KINDS]
    n_lib = sum(1 for _, _, where in pairs if re.fullmatch(r'_lib\.[A-Z0-9_]+', where))
    assert n_lib > 0
    print('%d constants, %d of them plain integers of _lib' % (len(pairs), n_lib))


# ------------------------------------------------------------------------------------------ the build and the documents
def test_build_lists_are_the_directories():
    assert sorted(build.SOURCES) == sorted(f for f in os.listdir(build.CSRC) if f.endswith(('.hip', '.cpp')))
    assert len(set(build.SOURCES)) == len(build.SOURCES) > 0
    assert os.path.samefile(build.INCLUDE, INCLUDE)
    assert 'for d in (CSRC, INCLUDE) for f in sorted(os.listdir(d)) if f.endswith(\'.h\')' in inspect.getsource(build.build)


def test_documents_name_the_surface():
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    readme = open(os.path.join(ROOT, 'README.md')).read()
    for header in HEADERS:
        assert header in integration, header
        assert re.search(r'(?<!\d)%d in `%s`' % (len(prototypes(header)), re.escape(header)), readme), header
    named = {name for name in _lib.SIGNATURES if re.search(r'\b%s\b' % name, integration)}
    assert UNDOCUMENTED <= set(_lib.SIGNATURES)
    assert not UNDOCUMENTED & named, 'now documented, take them out of UNDOCUMENTED: %s' % sorted(UNDOCUMENTED & named)
    missing = set(_lib.SIGNATURES) - named - UNDOCUMENTED
    assert not missing, 'INTEGRATION.md does not name %s' % sorted(missing)
    assert '%d entry points' % len(_lib.SIGNATURES) in integration


if __name__ == '__main__' and sys.argv[1:] == ['--record']:
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        rows = [' %s: %s' % (json.dumps(name), json.dumps(s)) for name, s in run_probe(tmp)[0].items()]
    open(LAYOUT_FILE, 'w').write('{\n' + ',\n'.join(rows) + '\n}\n')
