"""Drop-in check against the reference's model modules: with install_into_reference() the imports those modules make of
the operators resolve to OUR softsplat / euler modules (no cupy anywhere), and what the reference model holds is our
ModuleSoftsplat / EulerIntegration, whose call refuses CPU tensors.  The names the reference's model files import, and what
AnimatingSoftmaxSplating held and raised when it was built on them, are stored in tests/golden/reference_io.npz
(tools/make_golden_reference_checks.py); here a stand-in `models` package makes the same imports."""
import sys

import numpy as np
import pytest
import torch


def _stand_in_package(root, imports):
    """models/ with one module per reference model file, holding exactly the recorded operator imports."""
    files = {}
    for rec in imports:
        mod, src, names = rec.split("|")
        files.setdefault(mod, []).append(f"from {src} import {', '.join(names.split(','))}")
    for pkg in ("models", "models/projection"):
        (root / pkg).mkdir(parents=True, exist_ok=True)
        (root / pkg / "__init__.py").write_text("")
    for mod, lines in files.items():
        (root / (mod.replace(".", "/") + ".py")).write_text("\n".join(lines) + "\n")
    return sorted(files)


def test_reference_models_import_and_call_our_ops(tmp_path, golden_dir):
    import importlib
    import slr_sfs_amd as S
    g = np.load(f"{golden_dir}/reference_io.npz")
    imports = [str(s) for s in g["dropin_imports"]]
    assert any(s.endswith("|models|softsplat") for s in imports)
    assert any("|models.projection.euler_integration_manipulator|" in s for s in imports)
    saved = {k: v for k, v in sys.modules.items() if k == "models" or k.startswith("models.") or k == "cupy"}
    for k in saved:
        del sys.modules[k]
    mods = _stand_in_package(tmp_path, imports)
    sys.path.insert(0, str(tmp_path))
    try:
        ss, eim = S.install_into_reference()
        for mod in mods:
            m = importlib.import_module(mod)                          # does `from models import softsplat` & co.
            for rec in imports:
                name, src, names = rec.split("|")
                if name != mod:
                    continue
                for n in names.split(","):
                    ours = ss if src == "models" and n == "softsplat" else getattr(eim, n)
                    assert getattr(m, n) is ours, (mod, n)
        assert "cupy" not in sys.modules                              # nothing pulled cupy in
        cls, str_type = (str(s) for s in g["dropin_softsplater"])
        softsplater = getattr(ss, cls)(str_type)
        assert isinstance(softsplater, ss.ModuleSoftsplat) and softsplater.strType == "summation"
        assert getattr(eim, str(g["dropin_euler_integration"])) is eim.EulerIntegration
        # on a GPU-less box the reference's forward_flow ended in OUR operator's refusal of CPU tensors (same exception type as
        # the reference's own CPU branch, softsplat.py:418-419); the operator it holds refuses the same way
        raised = str(g["dropin_forward_flow_raises"])
        assert raised.startswith("NotImplementedError:") and "ROCm device" in raised
        with pytest.raises(NotImplementedError, match="ROCm device") as e:
            softsplater(torch.zeros(1, 65, 16, 16), torch.zeros(1, 2, 16, 16), None)
        assert f"{type(e.value).__name__}: {e.value}" == raised
    finally:
        sys.path.remove(str(tmp_path))
        for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
            del sys.modules[k]
        sys.modules.update(saved)
