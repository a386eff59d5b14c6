// Test harness (not product): mm355_dpdomain.h -- the int8 domain of U:ksw2_extd2_sse.c that mm355_dp.hip's row_class asks before it
// sends a gap fill to the plain-recurrence kernels -- compiled for the HOST with g++, so that tests/test_ksw_domain_model.py holds the
// product's own predicate against the oracle on the CPU.
#include "../../mappy-rs_amd/csrc/mm355_dpdomain.h"

extern "C" int dp_domain_host(int a, int b, int sc_ambi, int q, int e, int q2, int e2)
{
	return mm355_dp_int8_domain(a, b, sc_ambi, q, e, q2, e2)? 1 : 0;
}
