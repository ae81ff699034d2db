"""Prints the `_capi` adapters (functions that launch a kernel) that no case of tests/test_gpu_guard_*.py names.  Expected output:
the data-preparation adapters those files declare out of scope, nothing else.  `--table`: per adapter, the tests (or the helpers
tests share) of those files that name it.  Reads source text only; needs no GPU."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_OF_SCOPE = {'cosine_map', 'albedo', 'diffuse_base', 'remap_bilinear', 'uv_index_map', 'knn_indices', 'psnr_sums', 'resize_cv_linear',
                'gather_frames_u8', 'assemble_batch'}


def adapters():
    """Top-level public functions of _capi.py whose body launches (`_call`, `_call_det`, `_pack`) and that take a tensor."""
    src = open(os.path.join(ROOT, 'neural-light-transport_amd', '_capi.py')).read()
    names = []
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef) and not node.name.startswith('_'):
            body = ast.get_source_segment(src, node)
            if re.search(r'\b_call(_det)?\(', body) and not re.search(r'\b(tape|event|replay)', node.name):
                names.append(node.name)
    return names


def table():
    """{adapter: ['file::function', ...]}: the top-level functions of the guard files (tests, or the helpers tests share) naming it."""
    where = {}
    for f in sorted(glob.glob(os.path.join(ROOT, 'tests', 'test_gpu_guard_*.py'))):
        src = open(f).read()
        for node in ast.parse(src).body:
            if isinstance(node, ast.FunctionDef):
                body = ast.get_source_segment(src, node)
                for n in re.findall(r'\bC\.([a-z0-9_]+)\b', body):
                    fn = '%s::%s' % (os.path.basename(f)[len('test_gpu_guard_'):-3], node.name)
                    if fn not in where.setdefault(n, []):
                        where[n].append(fn)
    return where


def main():
    import sys
    text = ''.join(open(f).read() for f in sorted(glob.glob(os.path.join(ROOT, 'tests', 'test_gpu_guard_*.py'))))
    if '--table' in sys.argv:
        where = table()
        for n in adapters():
            if n in where:
                print('%-32s %s' % (n, ', '.join(where[n])))
        return []
    missing = [n for n in adapters() if not re.search(r'\bC\.%s\b' % re.escape(n), text)]
    for n in missing:
        print(n + ('   (out of scope)' if n in OUT_OF_SCOPE else ''))
    return sorted(set(missing) - OUT_OF_SCOPE)


if __name__ == '__main__':
    raise SystemExit(1 if main() else 0)
