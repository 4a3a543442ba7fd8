"""CPU: the drop-in claim of INTEGRATION.md is checked against the reference -- public signatures, Detector behaviour and the
monkey-patch recipe -- through what `python -m oracle.make_reference_fixtures` recorded from the reference's own Python
(tests/golden/reference_api.json / .npz)."""
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_public_signatures_and_integration_patch_against_the_reference():
    p = subprocess.run([sys.executable, str(ROOT / "tests" / "_ref_api_check.py")], capture_output=True, text=True, timeout=600)
    line = next((l for l in p.stdout.splitlines() if l.startswith("REF_API_JSON ")), None)
    assert line is not None, p.stdout[-2000:] + p.stderr[-4000:]
    problems = json.loads(line[len("REF_API_JSON "):])
    assert problems == [], "\n".join(problems)
