#!/bin/bash
# GPU-box round check: parity tests, then a full bench line, each under its own limit.
# Logs land in $RTREC_OUT_DIR (default: a fresh temporary folder, printed at the end).
set -o pipefail
O=${RTREC_OUT_DIR:-$(mktemp -d)}; mkdir -p $O
TAG=${1:-run}
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $O/${TAG}_pytest.log 2>&1 || { tail -40 $O/${TAG}_pytest.log; exit 1; }
tail -3 $O/${TAG}_pytest.log
timeout -k 10 300 python -u bench.py --full > $O/${TAG}_bench.json 2> $O/${TAG}_bench.err || { tail -30 $O/${TAG}_bench.err; exit 1; }
cat $O/${TAG}_bench.json
echo "logs: $O"
