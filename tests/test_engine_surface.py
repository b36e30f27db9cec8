"""The surface of nerf2mesh_amd/engine.py after batch preparation moved to engine_batches.py, the optimizer pass to engine_adam.py and the SDF
recipe to engine_sdf.py: the names tests, tools and bench.py reach are still found on the module and on Stage0Engine, the two lower layers
do not import the engine, and the learning-rate schedule is the one of main.py:239.  Host code only."""
import ast
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from nerf2mesh_amd import engine, engine_adam, engine_batches   # noqa: E402

MODULE_NAMES = "Stage0Engine lr_lambda peer_chunk_rows".split()
METHODS = """supported train_step mark_untrained sync_parameters ema_update averaged_parameters eval_psnr _lambda_mask _finish _lr_step _refresh
_sdf_buf""".split()


def test_module_names_are_still_there():
    assert [n for n in MODULE_NAMES if not hasattr(engine, n)] == []
    assert engine.lr_lambda is engine_adam.lr_lambda and engine.peer_chunk_rows is engine_adam.peer_chunk_rows


def test_engine_keeps_its_methods():
    cls = engine.Stage0Engine
    assert [m for m in METHODS if not callable(getattr(cls, m, None))] == []
    assert isinstance(cls.__dict__["supported"], staticmethod)
    assert isinstance(cls.__dict__["loss_acc"], property)


def _imports(module):
    """Module names the source of `module` imports, relative ones by their last component."""
    with open(module.__file__) as f:
        tree = ast.parse(f.read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[-1] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names |= {(node.module or "").split(".")[-1]} | ({a.name for a in node.names} if not node.module else set())
    return names


def test_lower_layers_do_not_import_the_engine():
    assert "engine" not in _imports(engine_batches)
    assert "engine" not in _imports(engine_adam)
    assert {"engine_batches", "engine_adam", "engine_sdf"} <= _imports(engine)


def test_lr_lambda_points():
    iters = 30000
    assert engine.lr_lambda(0, iters) == 0.01
    assert engine.lr_lambda(500, iters) == 0.01 + 0.99 * (500 / 500)
    assert abs(engine.lr_lambda(500, iters) - 1.0) < 1e-15
    assert engine.lr_lambda(501, iters) == 0.1 ** (1 / (iters - 500))
    assert engine.lr_lambda(iters, iters) == 0.1
