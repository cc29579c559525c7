set -o pipefail
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export TMPDIR=/tmp
O=${ORBHIP_OUT:-bench_out}
mkdir -p $O
for k in ${KS:-2 3 4}; do
timeout -k 10 300 python3 -u bench.py --full --no-cpu --steps 50 --c3-inflight $k > $O/infl.log 2>&1 || exit 1
grep -v amdgpu.ids $O/infl.log | tail -1 | python3 -c "
import json,sys; d=json.loads(sys.stdin.read()); e=d['extra']
print('inflight=$k', 'C3', e['c3_1280x720_b64_extract_match_frames_per_s'], e['c3_one_batch_at_a_time_frames_per_s'])"
done
