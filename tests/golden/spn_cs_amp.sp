* common-source stage of sp_cs_amp.sp with the noise token: port 1 at the gate source, port 2 the supply-side source behind RD
VIN g 0 DC 0.9 AC 1 PORTNUM 1 Z0 50
VDD vdd 0 DC 3 PORTNUM 2 Z0 100
RD vdd d 5k
CL d 0 1p
CGD g d 20f
M1 d g 0 n 10e-6 1e-6 2
.MODEL 2 VT 0.5 MU 3e-2 COX 6e-3 LAMBDA 0.05 CJ0 4.0e-14
.SP DEC 5 1meg 1g 1
