"""Reads include/mode_hip.h -- the header build.py compiles the library against -- so that the Python side restates none of it.

parse(text) -> Header(prototypes, signatures, constants, records):
  prototypes  name -> (return C type, [(C type, parameter name)]), C types normalised ('const float*', 'long long', 'mode_stream_t')
  signatures  name -> (ctypes restype, [ctypes argtypes])
  constants   every `#define MODE_* <integer expression over earlier constants>` and the members of the anonymous enum
  records     every `typedef struct`: name -> [(field, C type, array length or None)]
It knows the C this one header uses and no more; a type outside CTYPES is an error that names the entry."""
import collections
import ctypes
import os
import re

PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), 'include', 'mode_hip.h')
STREAM = 'mode_stream_t'
CTYPES = {'int': ctypes.c_int, 'int32_t': ctypes.c_int, 'unsigned': ctypes.c_uint, 'long long': ctypes.c_longlong, 'size_t': ctypes.c_size_t,
          'float': ctypes.c_float, 'double': ctypes.c_double, STREAM: ctypes.c_void_p}
_TYPE_WORDS = set(CTYPES) | {'*', 'const', 'long', 'void', 'char'}

Header = collections.namedtuple('Header', 'prototypes signatures constants records')


def ctype_of(c_type, entry, is_return=False):
  """The ctypes class of a normalised C type; `entry` names the prototype or record in the error for a type outside the map."""
  if c_type.endswith('*'):
    return ctypes.c_char_p if is_return and c_type == 'const char*' else ctypes.c_void_p
  if c_type not in CTYPES:
    raise TypeError('%s: no ctypes mapping for C type %r' % (entry, c_type))
  return CTYPES[c_type]


def _type(text):
  return ' '.join(re.findall(r'\w+|\*', text)).replace(' *', '*')


def _parameter(text):
  """'const float* const* device_ptrs' -> ('const float* const*', 'device_ptrs'); an unnamed one, 'int' -> ('int', '')."""
  words = re.findall(r'\w+|\*', text)
  name = words.pop() if len(words) > 1 and words[-1] not in _TYPE_WORDS else ''
  return _type(' '.join(words)), name


def _constants(src):
  out = {}
  for body in re.findall(r'\benum\s*\{(.*?)\}', src, re.S):
    out.update((k, int(v, 0)) for k, v in re.findall(r'(\w+)\s*=\s*(-?\w+)', body))
  for name, expr in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(MODE_\w+)[ \t]+(\S.*)$', src, re.M):
    text = re.sub(r'\b[A-Za-z_]\w*', lambda m: str(out.get(m.group(), '?')), expr)  # earlier constants by value
    if not re.fullmatch(r'(0[xX][0-9a-fA-F]+|\d+|[\s()+*-])+', text):
      raise ValueError('%s: %r is not an integer expression over earlier constants' % (name, expr.strip()))
    out[name] = int(eval(text, {'__builtins__': {}}))  # (integer literals, + - * and brackets only: checked above)
  return out


_FIELD = r'\w+(?:\s*\[\s*\w+\s*\])?'


def _records(src, constants):
  out = {}
  for body, name in re.findall(r'\btypedef\s+struct\s+\w*\s*\{(.*?)\}\s*(\w+)\s*;', src, re.S):
    out[name] = fields = []
    for line in filter(None, (s.strip() for s in body.split(';'))):  # `float mean[3], std[3]`: one type, several declarators
      m = re.fullmatch(r'([^,]*?[\s*])(%s(?:\s*,\s*%s)*)' % (_FIELD, _FIELD), line)
      if not m:
        raise ValueError('%s: cannot read the field declaration %r' % (name, line))
      for field, n in re.findall(r'(\w+)(?:\s*\[\s*(\w+)\s*\])?', m.group(2)):
        fields.append((field, _type(m.group(1)), constants[n] if n in constants else int(n, 0) if n else None))
  return out


def parse(text):
  src = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
  constants = _constants(src)
  records = _records(src, constants)
  # what is left after the typedefs, the enum, the preprocessor lines and `extern "C" {` are the prototypes
  src = re.sub(r'\btypedef\b[^;{]*(\{.*?\})?[^;]*;|\benum\s*\{.*?\}\s*;|^[ \t]*#[^\n]*|\bextern\s+"C"\s*\{', ' ', src, flags=re.S | re.M)
  prototype = r'([\w\s*]+?)\b(\w+)\s*\(([^()]*)\)\s*;'
  rest = re.sub(prototype, '', src).replace('}', '').strip()
  if rest:
    raise ValueError('the header holds something this reader does not know: %r' % rest[:80])
  prototypes, signatures = {}, {}
  for ret, name, params in re.findall(prototype, src):
    if name in prototypes:
      raise ValueError('%s is declared twice' % name)
    params = [] if params.strip() in ('', 'void') else [_parameter(p) for p in params.split(',')]
    prototypes[name] = (_type(ret), params)
    signatures[name] = (ctype_of(_type(ret), name, True), [ctype_of(t, name) for t, _ in params])
  return Header(prototypes, signatures, constants, records)


def load(path=PATH):
  try:
    with open(path) as f:
      text = f.read()
  except OSError as e:
    raise RuntimeError('the C-ABI header %s, which the binding is derived from, cannot be read: %s' % (path, e))
  return parse(text)


def structure(header, record, name=None, doc=None):
  """A ctypes.Structure with the fields of a record, in the header's names and order."""
  fields = []
  for field, c_type, n in header.records[record]:
    t = ctype_of(c_type, '%s.%s' % (record, field))
    fields.append((field, t if n is None else t * n))
  return type(name or record, (ctypes.Structure,), {'_fields_': fields, '__doc__': doc or 'struct %s as the header declares it.' % record})
