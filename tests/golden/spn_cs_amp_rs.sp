* the stage of spn_cs_amp.sp between terminations: port 1 driven from VIN behind RS, port 2 loaded by RL to the supply
VIN s 0 DC 0.9
RS s g 50
VDD vs 0 DC 3
RL vs vdd 100
RD vdd d 5k
CL d 0 1p
CGD g d 20f
M1 d g 0 n 10e-6 1e-6 2
.MODEL 2 VT 0.5 MU 3e-2 COX 6e-3 LAMBDA 0.05 CJ0 4.0e-14
.NOISE V(vdd) VIN DEC 5 1meg 1g
