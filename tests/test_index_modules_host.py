"""The index's host code in three modules (li.layout, li.index,
li.index_update): every name that was importable from li.index still is and is
the same object, the update methods keep their signatures, and li.layout needs
no torch.  No GPU."""
import inspect
import os
import subprocess
import sys

import li.index
import li.index_update
import li.layout

# every name some file of the tree imported from li.index before the split
IMPORTED = """DeviceIndex DeviceRouter Searcher RowSource BucketLayout IndexDescHolder default_chunk_rows
DEFAULT_CHUNK_ROWS DEFAULT_SLAB_ROWS DEFAULT_DIRECT_ROWS STAGING_MAX_BYTES check_tags eligible_counts check_stop
probe_stop_mask refine_eps bucket_topk bucket_topk_f64 bucket_range want_words merge_topk global_band replay
replay_device answer_buffer answer_views check ptr _inv_norm _as_torch _SEED_ROUND0
split_sample_fallback_count""".split()
MOVED = {li.layout: ("BucketLayout", "check_tags", "eligible_counts", "default_chunk_rows", "DEFAULT_CHUNK_ROWS"),
         li.index_update: ("DEFAULT_SLAB_ROWS", "DEFAULT_DIRECT_ROWS", "STAGING_MAX_BYTES")}
# the methods' parameters before the split: name, * for keyword-only, =default
SIGNATURES = {
    "add": "self rows labels ids=None tags=None inplace*=False slab_rows*=None direct_rows*=None timings*=None",
    "remove": "self ids inplace*=False slab_rows*=None direct_rows*=None timings*=None",
    "relabel": "self labels n_buckets=None inplace*=False timings*=None",
    "reserve": "self rows",
    "empty": "d n_buckets device*=None chunk_rows*=None capacity*=None tags*=None",
}


def test_every_imported_name_is_still_in_li_index():
    for name in IMPORTED:
        assert hasattr(li.index, name), name
    for module, names in MOVED.items():
        for name in names:
            assert getattr(li.index, name) is getattr(module, name), name
    assert li.index.DeviceIndex._sorted_by_bucket is li.index_update.sorted_by_bucket


def test_update_methods_keep_their_signatures():
    P = inspect.Parameter
    for name, want in SIGNATURES.items():
        params = inspect.signature(getattr(li.index.DeviceIndex, name)).parameters.values()
        assert all(p.kind in (P.POSITIONAL_OR_KEYWORD, P.KEYWORD_ONLY) for p in params), name
        got = " ".join(p.name + ("*" if p.kind == P.KEYWORD_ONLY else "")
                       + ("" if p.default is P.empty else f"={p.default!r}") for p in params)
        assert got == want, (name, got)


def test_layout_imports_without_torch():
    pkg = os.path.dirname(os.path.dirname(li.layout.__file__))
    code = ("import sys; sys.path.insert(0, %r); import li.layout; "
            "assert 'torch' not in sys.modules, 'li.layout pulled torch in'; "
            "assert li.layout.BucketLayout.from_labels([1, 0, 1], 2).order.tolist() == [1, 0, 2]" % pkg)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=60)


def test_new_modules_need_no_oracle():
    for module in (li.layout, li.index_update):
        src = open(module.__file__).read()
        assert "lmi_oracle" not in src and "import oracle" not in src, module.__name__
    # the dependency runs one way: li.index imports li.index_update
    assert "li.index" not in _module_level_imports(li.index_update)


def _module_level_imports(module):
    """Absolute names of what `module` imports at module level."""
    import ast
    out = []
    for node in ast.parse(open(module.__file__).read()).body:
        if isinstance(node, ast.ImportFrom):
            base = "li" if node.level == 1 else ""
            mod = ".".join(x for x in (base, node.module) if x)
            out += [mod] + [f"{mod}.{a.name}" for a in node.names]
        elif isinstance(node, ast.Import):
            out += [a.name for a in node.names]
    return out
