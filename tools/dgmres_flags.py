"""--ksp-type gmres|dgmres, --eigen K, --carry 0|1 for the solver experiment tools (late_phase.py, agg_profile.py): taken out of sys.argv
anywhere on the command line, so that the positional arguments keep their places."""
import sys


def _pop_flag(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        val = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return val
    return default


KSP_TYPE = _pop_flag('--ksp-type', 'gmres')        # gmres | dgmres (GMRES with deflated restarting, ksfd_set_deflation)
EIGEN = int(_pop_flag('--eigen', '8'))             # harmonic Ritz vectors kept across a restart
CARRY = int(_pop_flag('--carry', '0'))             # 1: the kept space also serves the later stages of a step attempt (default as -ksfd_dgmres_carry)
if KSP_TYPE not in ('gmres', 'dgmres'):
    sys.exit('--ksp-type must be gmres or dgmres')
