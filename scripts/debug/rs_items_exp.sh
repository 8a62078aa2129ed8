for it in ${ITEMS:-8 16}; do
  GSR_EXTRA_FLAGS="-DGSR_RS_ITEMS=$it" python gaussian-pcloud-render_amd/build.py --force > /dev/null 2>&1
  for vpc in ${VPCS:-12 1}; do
  python bench.py --full --no-cpu-baseline --no-per-view --views-per-call $vpc 2>/dev/null | python -c "
import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); k=d['kernels_ms_per_frame']; print('items $it vpc $vpc', d['value'], 'depth', k['depth_sort'], 'tile', k['tile_sort'])"
  done
done
