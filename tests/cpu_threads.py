"""Threads for the CPU float64 references of the GPU tests: the cores this process may actually use.

A container on a large host sees every core of the host in its affinity mask while a CPU quota holds it to a few; a torch thread
pool sized by the mask then runs many times oversubscribed, and a float64 reference that takes seconds takes minutes."""
import os


def usable_cores():
  """Affinity mask, capped by the cgroup CPU quota (v2 cpu.max or v1 cfs) and by OMP_NUM_THREADS where it is set."""
  n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
  try:
    with open('/sys/fs/cgroup/cpu.max') as f:
      quota, period = f.read().split()
    if quota != 'max':
      n = min(n, max(1, int(float(quota) / float(period))))
  except (OSError, ValueError):
    try:
      with open('/sys/fs/cgroup/cpu/cpu.cfs_quota_us') as f, open('/sys/fs/cgroup/cpu/cpu.cfs_period_us') as g:
        q, p = int(f.read()), int(g.read())
      if q > 0:
        n = min(n, max(1, q // p))
    except (OSError, ValueError):
      pass
  omp = os.environ.get('OMP_NUM_THREADS', '').strip()
  if omp.isdigit() and int(omp) > 0:
    n = min(n, int(omp))
  return max(1, n)
