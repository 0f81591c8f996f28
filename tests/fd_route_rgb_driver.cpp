// Prints what the route rule of a gradient batch (tamcmc-c_amd/csrc/fd_route.h: fd_route) gives with its trailing rgb_adjoint argument, for
// the cases named on the command line as "request gradient fd_windowed precision delta_geometry Nvars rgb rgb_adjoint" octuples, one line
// "code route" per case (route -1: refused), in the format of tests/fd_route_driver.cpp; tests/test_fd_route_rgb.py restates the rule.
#include <cstdio>
#include <cstdlib>

#include "../tamcmc-c_amd/csrc/fd_route.h"

int main(int argc, char **argv) {
    for (int i = 1; i + 7 < argc; i += 8) {
        int v[8];
        for (int k = 0; k < 8; k++) v[k] = std::atoi(argv[i + k]);
        tamcmc::FdRoute route = tamcmc::FdRoute::Brute;
        const int rc = tamcmc::fd_route((tamcmc::FdRequest)v[0], v[1], v[2], v[3], v[4] != 0, v[5], v[6] != 0, &route, v[7] != 0);
        std::printf("%d %d\n", rc, rc == TAMCMC_OK ? (int)route : -1);
    }
    std::printf("routes %d %d %d %d requests %d %d %d %d\n", (int)tamcmc::FdRoute::Brute, (int)tamcmc::FdRoute::Windowed,
                (int)tamcmc::FdRoute::Adjoint, (int)tamcmc::FdRoute::Rows, (int)tamcmc::FdRequest::FromOptions, (int)tamcmc::FdRequest::Adjoint,
                (int)tamcmc::FdRequest::Rows, (int)tamcmc::FdRequest::Tables);
    return 0;
}
